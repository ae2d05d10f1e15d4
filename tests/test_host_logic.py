"""Host-side logic of the drop-in wrappers on CPU (no GPU, no library calls): image-span bookkeeping for both
processor layouts, error behaviour, return layouts, EOS handling, seed bookkeeping, fp8 quantiser round trip; and the table of which slice
kernel a wide decode GEMV runs (the one test here that loads the built library: host calls only)."""
import os

import numpy as np
import pytest
import torch

from dropoutdecoding_amd import config as ddc
from dropoutdecoding_amd.vlm import DropoutVLM, lm_state_dict_from_hf


class StubEngine:
    """Plays DropoutEngine for the wrapper: emits a scripted token sequence."""
    device = torch.device("cpu")

    def __init__(self, script):
        self.script, self.n, self.calls = list(script), 0, []

    def prefill(self, embeds, start, L, first_step_ensemble=False, stream=None):
        self.calls.append(("prefill", tuple(embeds.shape), start, L))
        self.n = 1

    def generate(self, n_new, eos=None, dropout=True, **kw):
        eos = set(eos or [])
        out = []
        for t in self.script[:n_new]:
            out.append(t)
            if t in eos:
                break
        self.calls.append(("generate", n_new, tuple(sorted(eos)), dropout))
        return out

    def tokens(self):
        return self.script[:self.n]

    def vision_uncert_dict(self):
        return {"epis_uncert_per_token": np.zeros((1, 4), np.float32)}

    def topk(self):
        return np.zeros((4, 5), np.float32), np.zeros((4, 5), np.int32)


class Wrap(DropoutVLM):
    family = "llava-1.5"

    def _visual_embeds(self, pixel_values=None, **_):
        return torch.full((4, 8), 7.0)


def make(script=(5, 6, 9, 3, 2)):
    emb = torch.arange(20 * 8, dtype=torch.float32).reshape(20, 8)
    return Wrap(StubEngine(script), emb, image_token_index=19, eos_token_id=9)


def test_merge_single_placeholder_and_expanded_run():
    m = make()
    e1, s1 = m._merge(torch.tensor([[1, 19, 3]]), torch.full((4, 8), 7.0))
    e2, s2 = m._merge(torch.tensor([[1, 19, 19, 19, 19, 3]]), torch.full((4, 8), 7.0))
    assert s1 == s2 == 1 and e1.shape == e2.shape == (6, 8) and torch.equal(e1, e2)
    assert torch.equal(e1[1:5], torch.full((4, 8), 7.0)) and torch.equal(e1[0], m.embed_tokens[1]) and torch.equal(e1[5], m.embed_tokens[3])


@pytest.mark.parametrize("ids", [[[1, 2, 3]], [[1, 19, 19, 3]], [[19, 1, 19, 19, 19]]])
def test_merge_rejects_wrong_image_token_counts(ids):
    with pytest.raises(ValueError, match="number of image tokens"):
        make()._merge(torch.tensor(ids), torch.full((4, 8), 7.0))       # reference llava.py:134-138


def test_generate_surface_and_state():
    m = make()
    ids = torch.tensor([[1, 19, 3]])
    out = m.generate(input_ids=ids, attention_mask=torch.ones_like(ids), pixel_values=torch.zeros(1), max_new_tokens=5,
                     num_beams=1, pad_token_id=0)
    assert out.tolist() == [[1, 19, 3, 5, 6, 9]]                      # stops on the model's EOS (9), prompt ids first
    assert m.start_image_pos == [1] and m.end_image_pos == [4] and m.start_generation_pos == 6
    assert m.engine.calls[0] == ("prefill", (6, 8), 1, 4)
    assert m.image_features[1].shape == (1, 4, 5) and "epis_uncert_per_token" in m.vision_uncert_dict
    out = m.generate(input_ids=ids, pixel_values=torch.zeros(1), max_new_tokens=4, eos_token_id=[])
    assert out.tolist() == [[1, 19, 3, 5, 6, 9, 3]]                   # EOS ignored, exactly max_new_tokens
    m.original = True
    m.generate(input_ids=ids, pixel_values=torch.zeros(1), max_new_tokens=2)
    assert m.engine.calls[-1][3] is False                            # --original: stock greedy steps


def test_generate_rejects_what_the_reference_cannot_do():
    m = make()
    with pytest.raises(ValueError):
        m.generate(input_ids=torch.tensor([[1, 19], [1, 19]]), pixel_values=torch.zeros(1))      # batch 2
    with pytest.raises(ValueError):
        m.generate(input_ids=torch.tensor([[1, 19]]), pixel_values=torch.zeros(1), num_beams=3)
    with pytest.raises(ValueError):
        m.generate(input_ids=torch.tensor([[1, 19]]), pixel_values=torch.zeros(1), do_sample=True)


def test_instructblip_output_layout():
    from dropoutdecoding_amd.instructblip import CustomInstructBlipForConditionalGeneration as IB
    emb = torch.arange(20 * 8, dtype=torch.float32).reshape(20, 8)
    m = IB(StubEngine((5, 6, 9)), emb, hf_front=None, eos_token_id=9, config=None)
    m._visual_embeds = lambda **kw: torch.full((4, 8), 7.0)
    out = m.generate(input_ids=torch.tensor([[1, 3, 4]]), pixel_values=torch.zeros(1), max_new_tokens=8)
    assert out.tolist() == [[2, 5, 6, 9]]                             # BOS(2) + new ids only (instructblip.py:686-695)
    assert m.start_image_pos == [0] and m.end_image_pos == [3] and m.engine.calls[0] == ("prefill", (7, 8), 0, 4)


def test_effective_seed_is_the_last_imported_module():
    import importlib
    import dropoutdecoding_amd.instructblip as a
    import dropoutdecoding_amd.llava as b
    import dropoutdecoding_amd.llavanext as c
    for mod, seed in ((b, 24), (c, 506), (a, 5217)):                  # chair_test's import order (chair_test.py:9,12,19)
        importlib.reload(mod)
        assert ddc.effective_seed == seed == mod.seed
    import models.config
    assert models.config.settings is ddc.settings and ddc.settings["voting_numbers"]


def test_lm_state_dict_layouts():
    w = {k: torch.zeros(1) for k in ("language_model.model.embed_tokens.weight", "language_model.model.layers.0.mlp.up_proj.weight",
                                     "language_model.lm_head.weight", "vision_tower.x")}

    class M:
        def state_dict(self):
            return w
    sd = lm_state_dict_from_hf(M())
    assert set(sd) == {"model.embed_tokens.weight", "model.layers.0.mlp.up_proj.weight", "lm_head.weight"}
    w2 = {"model.language_model.embed_tokens.weight": torch.ones(1), "model.language_model.norm.weight": torch.ones(1),
          "model.vision_tower.y": torch.ones(1)}

    class M2:
        def state_dict(self):
            return w2
    sd2 = lm_state_dict_from_hf(M2())
    assert set(sd2) == {"model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"}     # tied head filled in


def test_fp8_quantiser_round_trip():
    from dropoutdecoding_amd.lm import dequantize_fp8, quantize_fp8
    w = torch.randn(32, 64, generator=torch.Generator().manual_seed(0)) * 0.05
    q, s = quantize_fp8(w)
    assert q.dtype == torch.uint8 and s.shape == (32,)
    d = dequantize_fp8(q, s)
    assert float((d - w).abs().max()) <= float(w.abs().max()) / 16 + 1e-9          # e4m3: 3 mantissa bits
    assert float(d.abs().max(dim=1).values.sub(w.abs().max(dim=1).values).abs().max()) < 1e-6   # row maxima are exact


def test_bench_gpus_n_starts_its_own_ranks_before_any_gpu_call(monkeypatch):
    """`python bench.py --gpus N` outside a launcher: N ranks through torch.distributed.run on 127.0.0.1, spawned as child processes
    before the parent touches the GPU; inside a launcher (WORLD_SIZE set) nothing is spawned."""
    import importlib
    import subprocess
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    calls = []
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: calls.append((cmd, env)) or 7)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU touched before the spawn")))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "2", "--warmup", "1"])
    assert bench.main() == 7                                     # the children's status is the parent's
    (cmd, env), = calls
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(os.path.join(root, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "2", "--warmup", "1"]
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_bench_options_full_and_dump_outputs():
    """The plain run's switches: --full and --dump-outputs exist, and a run without a timed step is refused before anything starts."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_bench_takes_its_committed_profile_from_the_rounds_own_files(tmp_path, monkeypatch):
    """`roofline.traffic` / `kernel_stats_avg_us` come from profiles/rNN_pmc_summary.json and rNN_kernel_stats.csv of the newest round (config 5:
    rNN_c5_*) — not from any other file that merely ends in the same words (round 4: a tool's r04_prefill_ab_*_kernel_stats.csv sorted last and
    the bench line carried a null)."""
    import importlib
    import json
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    bench = importlib.import_module("bench")
    prof = tmp_path / "profiles"
    prof.mkdir()
    kern = "k_gemv_slices_seq<9, 4, 16, 3, 0, 2>"
    for name, avg in (("r03_kernel_stats.csv", 48400.0), ("r04_kernel_stats.csv", 47850.0), ("r04_c5_kernel_stats.csv", 30390.0),
                      ("r04_prefill_ab_mistral_kernel_stats.csv", 1.0)):
        (prof / name).write_text('"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n'
                                 f'"void {kern}(SliceArgs)",10,{avg * 10},{avg},1.0,1,2,0.0\n')
    for name, rd in (("r03_pmc_summary.json", 1), ("r04_pmc_summary.json", 184000000), ("r04_c5_pmc_summary.json", 55000000)):
        (prof / name).write_text(json.dumps({"kernels": {f"void {kern}(SliceArgs)": {"hbm_read_bytes_per_launch": rd, "hbm_write_bytes_per_launch": 1000}}}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench._profile_files() == (os.path.join("profiles", "r04_pmc_summary.json"), os.path.join("profiles", "r04_kernel_stats.csv"))
    assert bench._profile_files("c5_") == (os.path.join("profiles", "r04_c5_pmc_summary.json"), os.path.join("profiles", "r04_c5_kernel_stats.csv"))
    got = bench.committed_profile(kern)
    assert got["stats_avg_us"] == 47.85 and got["traffic"] == 184001000 and got["stats_file"].endswith("r04_kernel_stats.csv")
    assert bench.committed_profile(kern, "c5_")["stats_avg_us"] == 30.39
    (prof / "r04_c5_kernel_stats.csv").unlink()                      # no config-5 trace this round: fall back to the default collection
    assert bench._profile_files("c5_")[1] == os.path.join("profiles", "r04_kernel_stats.csv")


def test_tensor_parallel_shards_reassemble_the_layer():
    """lm.tp_local_config / tp_shard_state_dict: head-aligned slices, d_ff padded to a multiple of 256 with zero rows / columns —
    the ranks' partial MLP and attention-output products add up to the un-sharded layer's."""
    import torch.nn.functional as F
    from dropoutdecoding_amd import lm
    cfg = lm.LMConfig(64, 512, 1280, 1, 4, 2, 128, 1e-5, 10000.0)
    g = torch.Generator().manual_seed(0)
    sd = {"model.embed_tokens.weight": torch.randn(64, 512, generator=g), "model.norm.weight": torch.ones(512), "lm_head.weight": torch.randn(64, 512, generator=g)}
    p = "model.layers.0."
    sd[p + "input_layernorm.weight"] = sd[p + "post_attention_layernorm.weight"] = torch.ones(512)
    sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.o_proj.weight"] = torch.randn(512, 512, generator=g), torch.randn(512, 512, generator=g)
    sd[p + "self_attn.k_proj.weight"], sd[p + "self_attn.v_proj.weight"] = torch.randn(256, 512, generator=g), torch.randn(256, 512, generator=g)
    sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = torch.randn(1280, 512, generator=g), torch.randn(1280, 512, generator=g)
    sd[p + "mlp.down_proj.weight"] = torch.randn(512, 1280, generator=g)
    local = lm.tp_local_config(cfg, 2)
    assert (local.num_heads, local.num_kv_heads, local.intermediate_size) == (2, 1, 768)      # 640 columns padded to 768
    x = torch.randn(5, 512, generator=g)
    full = F.linear(F.silu(F.linear(x, sd[p + "mlp.gate_proj.weight"])) * F.linear(x, sd[p + "mlp.up_proj.weight"]), sd[p + "mlp.down_proj.weight"])
    o_full = F.linear(x, sd[p + "self_attn.o_proj.weight"])
    part, o_part = 0, 0
    for r in range(2):
        sh = lm.tp_shard_state_dict(sd, cfg, r, 2)
        assert sh[p + "mlp.gate_proj.weight"].shape == (768, 512) and sh[p + "mlp.down_proj.weight"].shape == (512, 768)
        assert sh[p + "self_attn.q_proj.weight"].shape == (256, 512) and sh[p + "self_attn.k_proj.weight"].shape == (128, 512)
        assert sh["lm_head.weight"] is sd["lm_head.weight"]
        part = part + F.linear(F.silu(F.linear(x, sh[p + "mlp.gate_proj.weight"])) * F.linear(x, sh[p + "mlp.up_proj.weight"]), sh[p + "mlp.down_proj.weight"])
        o_part = o_part + F.linear(x[:, 256 * r:256 * (r + 1)], sh[p + "self_attn.o_proj.weight"])
    assert torch.allclose(part, full, rtol=1e-4, atol=1e-3) and torch.allclose(o_part, o_full, rtol=1e-4, atol=1e-3)
    with pytest.raises(ValueError):
        lm.tp_local_config(cfg, 4)                        # 2 kv heads do not split over 4 ranks


# ---- which slice kernel a 16- / 32- / 64- / 72-row decode GEMV runs (csrc/dd_gemv.hip plan_slices through dd_tools_gemv_plan) ----
# The 7B families' matrices as GemvArgs describes them: (epilogue, S = K / 32, n_tiles; EPI_SILU counts gate/up pairs).
_STORE, _RESID, _SILU, _QKV = 0, 1, 2, 3
_LLAVA = {"qkv": (_QKV, 128, 768), "o": (_RESID, 128, 256), "gate_up": (_SILU, 128, 688), "down": (_RESID, 344, 256)}     # d_ff 11008, 32 / 32 heads
_MISTRAL = {"qkv": (_QKV, 128, 384), "o": (_RESID, 128, 256), "gate_up": (_SILU, 128, 896), "down": (_RESID, 448, 256)}   # d_ff 14336, 32 / 8 heads
_LM_HEAD = (_STORE, 128, 2000)
_PART = 8 * 2000 * 9 * 128           # room for every case below
_KS, _SEQ = "k_gemv_slices<{}, {w}, {}, {}>", "k_gemv_slices_seq<{}, {w}, {}, 2>"
# {(model, matrix, planes): (kernel name with the weight-format argument left open, grid, partial sums per output) or None = no slice
# kernel}.  Names as the parent of the commit that introduced the plan printed them on an MI355X (dd_lm_time_gemv +
# dd_tools_last_gemv_kernel; lm_head from reading its ladders), grids from those ladders by hand: streaming workgroups + one for the rows'
# rstd where the operand carries the folded RMSNorm (every epilogue but the residual one).
_PLAN_16BIT = {
    ("llava", "qkv", 2): (_KS.format("2, 2, 8, 16, 16, 1", "3", "1", w="{w}"), 8 * 24 + 1, 8),        # 384 tile pairs, two per wave
    ("mistral", "qkv", 2): (_KS.format("2, 2, 8, 16, 16, 1", "3", "1", w="{w}"), 8 * 24 + 1, 8),      # 192 tile pairs, one per wave
    ("llava", "qkv", 4): (_KS.format("2, 4, 8, 16, 16, 1", "3", "1", w="{w}"), 193, 8),
    ("mistral", "qkv", 4): (_KS.format("2, 4, 8, 16, 16, 1", "3", "1", w="{w}"), 193, 8),
    ("llava", "qkv", 8): (_SEQ.format("8, 8, 16, 2", "3", w="{w}"), 4 * 48 + 1, 4),
    ("mistral", "qkv", 8): (_SEQ.format("8, 8, 16, 2", "3", w="{w}"), 4 * 24 + 1, 4),
    ("llava", "qkv", 9): (_SEQ.format("9, 4, 16, 2", "3", w="{w}"), 4 * 48 + 1, 4),
    ("mistral", "qkv", 9): (_SEQ.format("9, 4, 16, 2", "3", w="{w}"), 4 * 24 + 1, 4),
    ("llava", "o", 2): None, ("mistral", "o", 2): None, ("llava", "o", 4): None, ("mistral", "o", 4): None,
    ("llava", "o", 8): (_KS.format("1, 4, 8, 16, 16, 1", "1", "1", w="{w}"), 2 * 8 * 16, 8),           # two half passes of four planes
    ("mistral", "o", 8): (_KS.format("1, 4, 8, 16, 16, 1", "1", "1", w="{w}"), 2 * 8 * 16, 8),
    ("llava", "o", 9): (_KS.format("1, 9, 8, 16, 16, 1", "1", "0", w="{w}"), 8 * 16, 8),
    ("mistral", "o", 9): (_KS.format("1, 9, 8, 16, 16, 1", "1", "0", w="{w}"), 8 * 16, 8),
    ("llava", "gate_up", 2): (_KS.format("1, 2, 8, 16, 16, 2", "2", "1", w="{w}"), 4 * 64 + 1, 4),
    ("mistral", "gate_up", 2): (_KS.format("1, 2, 8, 16, 16, 2", "2", "1", w="{w}"), 4 * 64 + 1, 4),
    ("llava", "gate_up", 4): (_KS.format("1, 4, 8, 16, 16, 2", "2", "1", w="{w}"), 257, 4),
    ("mistral", "gate_up", 4): (_KS.format("1, 4, 8, 16, 16, 2", "2", "1", w="{w}"), 257, 4),
    ("llava", "gate_up", 8): (_SEQ.format("8, 8, 16, 3", "2", w="{w}"), 4 * 58 + 1, 4),                # 1376 tiles, three per wave
    ("mistral", "gate_up", 8): (_KS.format("1, 8, 8, 16, 16, 1", "2", "0", w="{w}"), 8 * 42 + 1, 8),   # 1792 tiles: single slices
    ("llava", "gate_up", 9): (_SEQ.format("9, 4, 16, 3", "2", w="{w}"), 4 * 58 + 1, 4),
    ("mistral", "gate_up", 9): (_KS.format("1, 9, 8, 16, 16, 1", "2", "0", w="{w}"), 8 * 32 + 1, 8),
    ("llava", "down", 2): (_KS.format("1, 2, 8, 43, 16, 1", "1", "0", w="{w}"), 256, 8),
    ("llava", "down", 4): (_KS.format("1, 4, 8, 43, 16, 1", "1", "0", w="{w}"), 256, 8),
    ("llava", "down", 8): (_KS.format("1, 8, 8, 43, 8, 1", "1", "0", w="{w}"), 256, 8),
    ("llava", "down", 9): (_KS.format("1, 9, 8, 43, 8, 1", "1", "0", w="{w}"), 256, 8),
    ("mistral", "down", 2): (_KS.format("1, 2, 8, 56, 16, 1", "1", "0", w="{w}"), 256, 8),
    ("mistral", "down", 4): (_KS.format("1, 4, 8, 56, 16, 1", "1", "0", w="{w}"), 256, 8),
    ("mistral", "down", 8): (_KS.format("1, 8, 8, 56, 8, 1", "1", "0", w="{w}"), 256, 8),
    ("mistral", "down", 9): (_KS.format("1, 9, 8, 56, 8, 1", "1", "0", w="{w}"), 256, 8),
    ("any", "lm_head", 2): None,
    ("any", "lm_head", 4): (_KS.format("1, 4, 8, 16, 16, 2", "0", "1", w="{w}"), 4 * 64 + 1, 4),
    ("any", "lm_head", 8): (_KS.format("1, 8, 8, 16, 16, 1", "0", "0", w="{w}"), 8 * 63 + 1, 8),
    ("any", "lm_head", 9): (_KS.format("1, 9, 8, 16, 16, 1", "0", "0", w="{w}"), 8 * 63 + 1, 8),
}
_PLAN_FP8 = {       # Mistral-7B, fp8 tiles: whole slices of 8 (K = 4096) or 28 (K = 14336) 64-k steps; at most one workgroup per CU
    ("qkv", 2): ("k_gemv_slices_fp8<2, 8, 2, 8, 0, 0>", 4 * 48 + 1, 4), ("o", 2): ("k_gemv_slices_fp8<2, 8, 2, 8, 0, 0>", 4 * 32, 4),
    ("gate_up", 2): ("k_gemv_slices_fp8<2, 8, 2, 8, 0, 0>", 4 * 64 + 1, 4), ("down", 2): ("k_gemv_slices_fp8<2, 28, 1, 7, 0, 0>", 8 * 32, 8),
    ("qkv", 4): ("k_gemv_slices_fp8<4, 8, 2, 8, 0, 0>", 4 * 48 + 1, 4), ("o", 4): ("k_gemv_slices_fp8<4, 8, 2, 8, 0, 0>", 4 * 32, 4),
    ("gate_up", 4): ("k_gemv_slices_fp8<4, 8, 2, 8, 0, 0>", 4 * 64 + 1, 4), ("down", 4): ("k_gemv_slices_fp8c<4, 28, 7, 7, 0>", 8 * 32, 8),
    ("qkv", 8): ("k_gemv_slices_fp8<8, 8, 1, 8, 0, 0>", 8 * 32 + 1, 8), ("o", 8): ("k_gemv_slices_fp8<8, 8, 1, 8, 0, 0>", 8 * 32, 8),
    ("gate_up", 8): ("k_gemv_slices_fp8<8, 8, 1, 8, 0, 0>", 8 * 32 + 1, 8), ("down", 8): ("k_gemv_slices_fp8c<8, 28, 4, 4, 0>", 8 * 32, 8),
    ("qkv", 9): ("k_gemv_slices_fp8<9, 8, 1, 8, 0, 6>", 8 * 32 + 1, 8), ("o", 9): ("k_gemv_slices_fp8<9, 8, 1, 8, 0, 6>", 8 * 32, 8),
    ("gate_up", 9): ("k_gemv_slices_fp8<9, 8, 1, 8, 0, 6>", 8 * 32 + 1, 8), ("down", 9): ("k_gemv_slices_fp8c<9, 28, 4, 4, 0>", 8 * 32, 8),
}


def _gemv_plan(lib, epi, planes, wq, wf, S, n_tiles, half_planes=0, part_floats=_PART):
    import ctypes
    name, grid, np_ = ctypes.create_string_buffer(96), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.dd_tools_gemv_plan(epi, planes, wq, wf, S, n_tiles, half_planes, part_floats, name, len(name), ctypes.byref(grid), ctypes.byref(np_))
    assert rc in (0, 1), (rc, lib.dd_last_error())
    return (name.value.decode(), grid.value, np_.value) if rc == 0 else None


def test_gemv_plan_names_grid_and_finish_for_the_7b_families():
    from dropoutdecoding_amd import _lib, build
    build.build()
    lib = _lib.load_tools()                                   # plain dlopen + host calls: the plan makes no HIP call
    shapes = {"llava": _LLAVA, "mistral": _MISTRAL, "any": {"lm_head": _LM_HEAD}}
    for wf in (0, 1):
        for (model, matrix, planes), want in _PLAN_16BIT.items():
            got = _gemv_plan(lib, *((shapes[model][matrix][0], planes, 0, wf) + shapes[model][matrix][1:]))
            assert got == (want and (want[0].format(w=wf),) + want[1:]), (model, matrix, planes, wf)
        # half planes (K <= 4: two sequences per operand plane) ride the same eight- / nine-plane kernels
        for planes, hp in ((8, 8), (9, 7)):
            for model in ("llava", "mistral"):
                for matrix, (epi, S, nt) in shapes[model].items():
                    want = _PLAN_16BIT[(model, matrix, planes)]
                    assert _gemv_plan(lib, epi, planes, 0, wf, S, nt, half_planes=hp) == (want[0].format(w=wf),) + want[1:], (model, matrix, planes, hp)
    for (matrix, planes), want in _PLAN_FP8.items():
        assert _gemv_plan(lib, _MISTRAL[matrix][0], planes, 1, 0, *_MISTRAL[matrix][1:]) == want, (matrix, planes)
    for planes in (2, 4, 8, 9):
        assert _gemv_plan(lib, _RESID, planes, 1, 0, 344, 256) is None                   # fp8, K = 11008: not whole 64-k steps per wave
        for model in (_LLAVA, _MISTRAL):
            for epi, S, nt in list(model.values()) + [_LM_HEAD]:
                assert _gemv_plan(lib, epi, planes, 2, 0, S, nt) is None                 # MXFP4: no slice kernels
        assert _gemv_plan(lib, _QKV, planes, 0, 0, 128, 63) is None                      # fewer than 64 tiles
        assert _gemv_plan(lib, _SILU, planes, 0, 0, 128, 31) is None                     # (62 gate/up tiles)
        assert _gemv_plan(lib, _QKV, planes, 1, 0, 128, 63) is None
    # the partial-sum buffer: eight slabs of tiles x planes x 128 floats (slice pairs up to four planes: four), not one float less
    for epi, planes, S, nt, need in ((_QKV, 9, 128, 768, 8 * 768 * 9 * 128), (_QKV, 8, 128, 768, 8 * 768 * 8 * 128), (_SILU, 4, 128, 688, 4 * 1376 * 4 * 128),
                                     (_QKV, 2, 128, 768, 8 * 768 * 2 * 128), (_RESID, 4, 344, 256, 8 * 256 * 4 * 128)):
        assert _gemv_plan(lib, epi, planes, 0, 0, S, nt, part_floats=need) is not None, (epi, planes)
        assert _gemv_plan(lib, epi, planes, 0, 0, S, nt, part_floats=need - 1) is None, (epi, planes)
    assert _gemv_plan(lib, _QKV, 9, 1, 0, 128, 384, part_floats=8 * 384 * 9 * 128 - 1) is None
    assert _gemv_plan(lib, _SILU, 2, 1, 0, 128, 896, part_floats=4 * 1792 * 2 * 128 - 1) is None
