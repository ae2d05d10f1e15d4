"""Generation record (include/dropdec.h "Generation record", csrc/dd_record.hip): per-token ensemble outcome, softmax summaries and the
score rows, written on the device by the step itself.

Tolerances.  Integers (tokens, winner, member ids, masked_numbers, base argmax, votes, top-8 ids) are exact.  The score rows are held to
the logits tolerance of tests/test_gpu_engine.py (`close`: 1e-3 of the largest |logit| of the oracle's row); x[t] - logsumexp(x) moves by at
most 2 * max|dx| when x moves by dx, so the log-probabilities are held to twice that.  The kernel's own arithmetic is compared with a float64
recomputation from the row IT recorded: lse and logprob within 1e-5 absolute on |logits| <= 32 (a fixed tree over <= 32064 non-positive
exponents: relative error ~ (log2 V + 4) * 2^-24 ~ 1e-6, plus the rounding of x - max ~ 2e-6), the entropy within that times log V."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.decode_ref import FAMILY_IBLIP, FAMILY_LLAVA, FAMILY_NEXT, RefDecoder
from oracle.lm_ref import LMConfig as RefCfg, random_weights

K8 = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
K4 = [0.1, 0.3, 0.5, 0.7]
SMALL = (512, 256, 512, 2, 2, 2, 128, 1e-5, 10000.0)


@pytest.fixture(scope="module")
def E():
    from dropoutdecoding_amd import build
    build.build()
    from dropoutdecoding_amd import lm
    return lm


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _engine(E, g, family, seed=None, max_seq=256):
    v, d, f, nl, nh, nkv, hd = [int(x) for x in g["cfg"]]
    rcfg = RefCfg(v, d, f, nl, nh, nkv, hd, float(g["rms_eps"]), float(g["rope_theta"]))
    w = random_weights(rcfg, int(g["wseed"]), float(g["std"]))
    cfg = E.LMConfig(v, d, f, nl, nh, nkv, hd, float(g["rms_eps"]), float(g["rope_theta"]))
    eng = E.DropoutEngine(cfg, family=family, max_seq=max_seq, max_visual=int(g["span_len"]) + 8, seed=seed)
    eng.load_state_dict(w)
    return eng, rcfg, w


def _small(E, family=FAMILY_LLAVA, seed=11, wseed=17, max_seq=160, max_visual=40, **kw):
    w = random_weights(RefCfg(*SMALL), wseed, 0.05)
    eng = E.DropoutEngine(E.LMConfig(*SMALL), family=family, max_seq=max_seq, max_visual=max_visual, seed=seed, **kw)
    eng.load_state_dict(w)
    return eng, w


def _cpu(rec):
    return {k: v.cpu().numpy().copy() for k, v in rec.items()}


def _log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max()
    return x - (m + math.log(np.exp(x - m).sum()))


def _top8(x):
    x = np.asarray(x)
    order = np.lexsort((np.arange(x.size), -x.astype(np.float64)))       # value descending, equal values: lowest id first
    return order[:8]


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------------
GOLD = {FAMILY_LLAVA: "g5_llava_k3.npz", FAMILY_NEXT: "g5_next_k4.npz", FAMILY_IBLIP: "g5_iblip_k3.npz"}


@pytest.mark.parametrize("K", [3, 8, 0])
@pytest.mark.parametrize("family", [FAMILY_LLAVA, FAMILY_NEXT, FAMILY_IBLIP])
def test_record_against_the_oracle(E, golden_dir, family, K):
    """The 24-step oracle runs of tests/test_gpu_engine.py (same fixtures, seed, step count); K = 0 is dropout=False."""
    g = _load(golden_dir, GOLD[family])
    probs = K8[:K]
    eng, rcfg, w = _engine(E, g, family, seed=77)
    ref = RefDecoder(family, rcfg, w, probs, seed=77, dropout=K > 0)
    emb = torch.from_numpy(g["embeds"])
    s0, L = int(g["span_start"]), int(g["span_len"])
    n_new = 25
    want = ref.generate(emb, s0, L, n_new)
    eng.attach_record(n_new, scores=True)
    eng.prefill(emb.cuda(), s0, L)
    for s in range(n_new - 1):
        eng.decode_step(probs, dropout=K > 0)
    assert eng.tokens() == want
    r = _cpu(eng.record())
    assert r["tokens"].tolist() == want and r["scores"].shape == (n_new, rcfg.vocab_size)
    worst = {"scores": 0.0, "logprob": 0.0, "base_logprob": 0.0}

    def check(i, tok, logits, base_logits):
        tol = 1e-3 * float(np.abs(np.asarray(logits, np.float64)).max())          # test_gpu_engine.close
        err = float(np.abs(r["scores"][i].astype(np.float64) - np.asarray(logits, np.float64)).max())
        worst["scores"] = max(worst["scores"], err / tol)
        assert err <= tol, f"record {i}: score row off by {err:.3g} (tolerance {tol:.3g})"
        for key, lg, name in (("token_logprobs", logits, "logprob"), ("base_token_logprobs", base_logits, "base_logprob")):
            t2 = 2e-3 * float(np.abs(np.asarray(lg, np.float64)).max())
            e2 = abs(float(r[key][i]) - float(_log_softmax64(lg)[tok]))
            worst[name] = max(worst[name], e2 / t2)
            assert e2 <= t2, f"record {i}: {key} off by {e2:.3g} (tolerance {t2:.3g})"

    # record 0: the prefill's greedy token, no ensemble
    last = ref.prefill_logits[-1].numpy()
    assert r["winner"][0] == -1 and r["K"][0] == 0 and r["votes"][0] == 0 and r["base_tokens"][0] == want[0]
    check(0, want[0], last, last)
    for i, sr in enumerate(ref.records, start=1):
        info = f"record {i}"
        assert r["tokens"][i] == sr.token and r["base_tokens"][i] == sr.base_argmax, info
        if K > 0:
            assert r["winner"][i] == sr.winner and r["K"][i] == K, info
            assert r["member_tokens"][i].tolist() == sr.member_argmax, info
            assert r["masked_numbers"][i].tolist() == sr.masked_numbers, info
            voted = sr.member_argmax[sr.winner]
            assert r["votes"][i] == sum(1 for a in sr.member_argmax if a == voted), info
        else:
            assert r["winner"][i] == -1 and r["K"][i] == 0 and r["votes"][i] == 0 and r["member_tokens"].shape[1] == 0, info
        check(i, sr.token, sr.logits, sr.base_logits)
    warnings.warn(f"record vs oracle ({family}, K={K}): worst error / tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    eng.close()


# ---- 2. the kernel's own arithmetic ----------------------------------------------------------------------------------------------------
def test_kernel_arithmetic_against_float64_of_its_own_rows(E, golden_dir):
    g = _load(golden_dir, GOLD[FAMILY_LLAVA])
    eng, rcfg, w = _engine(E, g, FAMILY_LLAVA, seed=77)
    n_new = 25
    eng.attach_record(n_new, scores=True)
    eng.prefill(torch.from_numpy(g["embeds"]).cuda(), int(g["span_start"]), int(g["span_len"]))
    for s in range(n_new - 1):
        eng.decode_step(K8)
    r = _cpu(eng.record())
    V = rcfg.vocab_size
    worst = {"max": 0.0, "lse": 0.0, "logprob": 0.0, "entropy": 0.0, "top_logit": 0.0, "absmax": 0.0}
    for i in range(n_new):
        x = r["scores"][i].astype(np.float64)
        worst["absmax"] = max(worst["absmax"], float(np.abs(x).max()))
        ls = _log_softmax64(x)
        lse = float(x[r["tokens"][i]] - ls[r["tokens"][i]])
        ent = float(-(np.exp(ls) * ls).sum())
        assert r["top_ids"][i].tolist() == _top8(r["scores"][i]).tolist(), f"record {i}: top-8 ids"
        np.testing.assert_array_equal(r["top_logits"][i], r["scores"][i][r["top_ids"][i]])
        assert r["max_logit"][i] == r["scores"][i].max()
        worst["lse"] = max(worst["lse"], abs(float(r["lse"][i]) - lse))
        worst["logprob"] = max(worst["logprob"], abs(float(r["token_logprobs"][i]) - float(ls[r["tokens"][i]])))
        worst["entropy"] = max(worst["entropy"], abs(float(r["entropy"][i]) - ent))
        worst["top_logit"] = max(worst["top_logit"], float(np.abs(r["top_logprobs"][i] - (r["top_logits"][i].astype(np.float64) - lse)).max()))
    warnings.warn(f"record kernel vs float64 of its own rows (V={V}, max |logit| {worst['absmax']:.3g}): max abs error lse {worst['lse']:.3g}, "
                  f"logprob {worst['logprob']:.3g}, entropy {worst['entropy']:.3g}, top_logprobs {worst['top_logit']:.3g}")
    assert worst["absmax"] <= 32
    assert worst["lse"] <= 1e-5 and worst["logprob"] <= 1e-5
    assert worst["entropy"] <= 1e-5 * math.log(V)
    eng.close()


def test_top8_with_tied_values_takes_the_lowest_ids_first(E):
    """A constructed row with tied values: the second half of lm_head repeats the first, so logit v + 256 is logit v bit for bit and every
    one of the eight largest values occurs twice."""
    w = random_weights(RefCfg(*SMALL), 17, 0.05)
    w = dict(w)
    head = w["lm_head.weight"].clone()
    head[256:] = head[:256]
    w["lm_head.weight"] = head
    eng = E.DropoutEngine(E.LMConfig(*SMALL), family=FAMILY_LLAVA, max_seq=160, max_visual=40, seed=11)
    eng.load_state_dict(w)
    emb = torch.randn(58, 256, generator=torch.Generator().manual_seed(3)).cuda()
    eng.attach_record(6, scores=True)
    eng.prefill(emb, 4, 40)
    for s in range(2):
        eng.decode_step(dropout=False)             # K = 0: the recorded row is the un-masked pass' own row
    for s in range(3):
        eng.decode_step([0.3, 0.5, 0.7])
    r = _cpu(eng.record())
    for i in range(6):
        row = r["scores"][i]
        np.testing.assert_array_equal(row[:256], row[256:], err_msg="the constructed row has no ties")
        want = _top8(row)
        assert want.tolist() == [j for v in _top8(row[:256])[:4] for j in (v, v + 256)]
        assert r["top_ids"][i].tolist() == want.tolist(), f"record {i}"
        np.testing.assert_array_equal(r["top_logits"][i], row[want])
        assert r["tokens"][i] == want[0]            # argmax: the first of equal maxima, as torch.argmax
    eng.close()


# ---- 3. observation changes nothing ----------------------------------------------------------------------------------------------------
def test_recording_changes_no_result(E):
    outs = []
    for rec in (False, True):
        eng, w = _small(E)
        emb = torch.randn(58, 256, generator=torch.Generator().manual_seed(3)).cuda()
        if rec:
            eng.attach_record(16, scores=True)
        eng.prefill(emb, 4, 40)
        for s in range(12):
            eng.decode_step([0.3, 0.5, 0.7])
        st = eng.last_step()
        outs.append((eng.tokens(), eng.logits().copy(), eng.base_logits().copy(), eng.kv_sums().copy(), st["drop"].copy(), st["keep"].copy(),
                     eng.rng.rand(8).cpu().numpy().copy()))
        eng.close()
    assert outs[0][0] == outs[1][0]
    for a, b, what in zip(outs[0][1:], outs[1][1:], ("logits", "un-masked logits", "KV sums", "masks", "keep set", "next uniforms")):
        np.testing.assert_array_equal(a, b, err_msg=what)


# ---- 4. lane = solo --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lanes,probs,form", [(16, K8, "rider"), (28, K4, "half planes")])
def test_lane_records_equal_solo_records_bytewise(E, n_lanes, probs, form):
    """The shapes of the lane-vs-solo tests of tests/test_gpu_rider.py / test_gpu_half_planes.py (7B widths, two layers, fp16 cache)."""
    d = 4096
    cfg = E.LMConfig(2048, d, 11008, 2, 32, 32, 128, 1e-5, 10000.0)
    L, n_new = 24, 7
    engines = []
    for i in range(n_lanes):
        engines.append(E.DropoutEngine(cfg, family=FAMILY_LLAVA, max_seq=L + 96, max_visual=L, seed=50 + i, kv_format="fp16",
                                       share_weights_with=engines[0] if engines else None))
    engines[0].load_synthetic(seed=3, std=0.02)
    gen = torch.Generator().manual_seed(9)
    embs = [(torch.randn(L + 6 + (i % 5), d, generator=gen) * 0.5).cuda() for i in range(n_lanes)]
    spans = [(2 + (i % 3), L) for i in range(n_lanes)]
    for e, emb, sp in zip(engines, embs, spans):
        e.attach_record(n_new, scores=True)
        e.prefill(emb, *sp)
    toks = E.EngineGroup(engines).generate(n_new, eos=[], mprobs=probs)
    recs = [_cpu(e.record()) for e in engines]
    assert all(len(t) == n_new for t in toks) and len({tuple(t) for t in toks}) > 1
    for li in range(n_lanes):
        e = engines[li]
        e.rng.manual_seed(50 + li)
        e.attach_record(n_new, scores=True)
        e.prefill(embs[li], *spans[li])
        assert e.generate(n_new, eos=[], mprobs=probs) == toks[li], f"{form}: lane {li}"
        solo = e.record()
        assert torch.equal(solo["raw"].cpu(), torch.from_numpy(recs[li]["raw"])), f"{form}: record bytes of lane {li}"
        assert torch.equal(solo["scores"].cpu(), torch.from_numpy(recs[li]["scores"])), f"{form}: score rows of lane {li}"
        assert recs[li]["tokens"].tolist() == toks[li]
    for e in reversed(engines):
        e.close()


# ---- 5. graph = eager, speculation modes -------------------------------------------------------------------------------------------------
def test_record_bytes_do_not_depend_on_graphs_or_speculation(E):
    from dropoutdecoding_amd import _lib
    lib = _lib.load()
    emb = torch.randn(58, 256, generator=torch.Generator().manual_seed(3)).cuda()
    probs = [0.3, 0.5, 0.7]
    runs = {}

    def run(tag, step, spec="default"):
        eng, w = _small(E)
        eng.set_speculation(spec)
        eng.attach_record(16, scores=True)
        eng.prefill(emb, 4, 40)
        for s in range(14):                                   # T: 58 -> 72 crosses the 64-key tile boundary (a new graph)
            getattr(eng, step)(probs)
        r = eng.record()
        runs[tag] = (eng.tokens(), r["raw"].cpu(), r["scores"].cpu())
        eng.close()

    try:
        for graph in (0, 1):
            lib.dd_set_tuning(8, graph)
            run(f"graph {graph}", "decode_step")
    finally:
        lib.dd_set_tuning(8, 1)
    for spec in ("never", "always", "adaptive"):
        for step in ("decode_step", "decode_step_sync"):
            run(f"{spec} {step}", step, spec)
    base = runs["graph 0"]
    assert len(base[0]) == 15
    for tag, got in runs.items():
        assert got[0] == base[0], tag
        assert torch.equal(got[1], base[1]), f"{tag}: record bytes"
        assert torch.equal(got[2], base[2]), f"{tag}: score rows"


# ---- 6. EOS and capacity ---------------------------------------------------------------------------------------------------------------
def test_steps_past_an_eos_and_past_the_capacity_write_nothing(E):
    emb = torch.randn(58, 256, generator=torch.Generator().manual_seed(3)).cuda()
    probs = [0.3, 0.5, 0.7]
    eng, w = _small(E)
    eng.prefill(emb, 4, 40)
    plain = eng.generate(14, eos=[], mprobs=probs)
    stop = next(i for i in range(3, 14) if plain[i] not in plain[:i])          # an id first emitted mid-way
    eos = plain[stop]
    eng.rng.manual_seed(11)
    eng.attach_record(14, scores=True)
    eng._rec_buf.fill_(0xFF)
    eng._rec_scores.view(torch.uint8).fill_(0xFF)
    torch.cuda.synchronize()
    eng.prefill(emb, 4, 40)
    eng.set_eos([eos])
    for s in range(13):                                       # queued without a look at the tokens: steps run past the EOS step
        eng.decode_step(probs)
    n = eng.n_tokens()
    assert n == stop + 1 and eng.tokens() == plain[:n]
    raw, sc = eng._rec_buf.cpu(), eng._rec_scores.view(torch.uint8).cpu()
    assert eng.record()["tokens"].cpu().tolist() == plain[:n]
    assert bool((raw[n:] == 0xFF).all()) and bool((sc[n:] == 0xFF).all()), "a step past the EOS wrote into the ring"
    assert not bool((raw[:n] == 0xFF).all(dim=1).any()), "a slot of an emitted token was left unwritten"
    # capacity smaller than the tokens generated
    cap = 5
    eng.set_eos([])
    eng.rng.manual_seed(11)
    eng.attach_record(cap, scores=True)
    eng.prefill(emb, 4, 40)
    assert eng.generate(14, eos=[], mprobs=probs) == plain
    r = eng.record()
    assert r["tokens"].cpu().tolist() == plain[:cap] and r["scores"].shape[0] == cap
    eng.detach_record()
    # the same through the C-ABI with a ring of `cap` records at the front of larger 0xFF-filled buffers: the rest stays untouched
    from dropoutdecoding_amd import _lib
    nb, V = _lib.record_dtype().itemsize, 512
    big = torch.full((14, nb), 0xFF, dtype=torch.uint8, device="cuda")
    big_sc = torch.full((14, 4 * V), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng._ck(eng.lib.dd_lm_set_record(eng._h, big.data_ptr(), cap, big_sc.data_ptr(), V, eng._s()), "dd_lm_set_record")
    eng.rng.manual_seed(11)
    eng.prefill(emb, 4, 40)
    assert eng.generate(14, eos=[], mprobs=probs) == plain
    torch.cuda.synchronize()
    assert bool((big[cap:] == 0xFF).all()) and bool((big_sc[cap:] == 0xFF).all()), "a token past the capacity was recorded"
    assert torch.equal(big[:cap].cpu(), r["raw"].cpu()) and torch.equal(big_sc[:cap].cpu(), r["scores"].contiguous().view(torch.uint8).cpu())
    eng._ck(eng.lib.dd_lm_set_record(eng._h, None, 0, None, 0, eng._s()), "dd_lm_set_record")
    eng.close()


# ---- 7. prefix reuse and re-prefill ------------------------------------------------------------------------------------------------------
def test_truncate_and_extend_start_again_at_slot_zero(E):
    probs = [0.3, 0.5, 0.7]
    gen = torch.Generator().manual_seed(5)
    head, tail1, tail2 = (torch.randn(n, 256, generator=gen).cuda() for n in (46, 6, 9))
    eng, w = _small(E)
    eng.attach_record(8, scores=True)
    eng.prefill(torch.cat([head, tail1]), 4, 40)
    eng.generate(8, eos=[], mprobs=probs)
    first = _cpu(eng.record())
    eng.truncate(46)
    eng.prefill_extend(tail2)
    toks = eng.generate(6, eos=[], mprobs=probs)
    second = _cpu(eng.record())
    assert second["tokens"].tolist() == toks and len(toks) == 6 and first["tokens"].shape[0] == 8
    # the same second prompt, decoded from a fresh truncate + extend on a fresh engine with the rng where it was
    eng2, _ = _small(E)
    eng2.attach_record(8, scores=True)
    eng2.prefill(torch.cat([head, tail1]), 4, 40)
    eng2.generate(8, eos=[], mprobs=probs)
    eng2.detach_record()
    eng2.attach_record(6, scores=True)
    eng2.truncate(46)
    eng2.prefill_extend(tail2)
    assert eng2.generate(6, eos=[], mprobs=probs) == toks
    fresh = _cpu(eng2.record())
    np.testing.assert_array_equal(fresh["raw"], second["raw"])
    np.testing.assert_array_equal(fresh["scores"], second["scores"])
    assert second["winner"][0] == -1 and second["K"][0] == 0
    eng.close()
    eng2.close()


# ---- 8. drop-in surface ----------------------------------------------------------------------------------------------------------------
def _tiny_llava():
    from transformers import CLIPVisionConfig, LlamaConfig, LlavaConfig, LlavaForConditionalGeneration
    torch.manual_seed(0)
    vc = CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2,
                          image_size=56, patch_size=14, projection_dim=16)
    tc = LlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                     num_key_value_heads=2, head_dim=128, max_position_embeddings=512, tie_word_embeddings=False)
    cfg = LlavaConfig(vision_config=vc, text_config=tc, image_token_index=511, vision_feature_layer=-2,
                      vision_feature_select_strategy="default")
    hf = LlavaForConditionalGeneration(cfg).eval()
    with torch.no_grad():
        for p_ in hf.parameters():
            p_.copy_(p_.to(torch.bfloat16).float())
        for n, p in hf.named_parameters():
            if "language_model" in n or "lm_head" in n:
                p.mul_(2.5)
    return hf


def test_generate_surface_returns_scores_and_the_record(E):
    from dropoutdecoding_amd import config as ddc
    from dropoutdecoding_amd.vlm import GroupPipeline, generate_group
    import models.llava as ML
    hf = _tiny_llava()
    saved = list(ddc.settings["voting_numbers"])
    try:
        ddc.settings["voting_numbers"] = [0.3, 0.5, 0.7]
        ddc._module_imported(24)
        m = ML.CustomLlavaForConditionalGeneration.from_hf_model(hf, max_new_tokens=16)
        prompts = [torch.tensor([[1, 17, 511, 45, 6, 7, 99]]), torch.tensor([[1, 511, 8, 9]]), torch.tensor([[1, 3, 4, 5, 511, 77]])]
        imgs = [(prompts[i % 3], torch.randn(1, 3, 56, 56, generator=torch.Generator().manual_seed(40 + i))) for i in range(6)]
        p, v = imgs[0]
        plain = m.spawn_lane().generate(input_ids=p, pixel_values=v, max_new_tokens=7, eos_token_id=[], output_scores=True)
        assert torch.is_tensor(plain)                                         # the two output_* keywords alone change nothing (HF)
        lane = m.spawn_lane()
        out = lane.generate(input_ids=p, pixel_values=v, max_new_tokens=7, eos_token_id=[], return_dict_in_generate=True, output_scores=True)
        assert torch.equal(out.sequences, plain) and torch.equal(out["sequences"], plain)
        assert len(out.scores) == 7 and out.scores[0].shape == (1, 512) and out.logits is None
        rec = out.dropout_record
        assert rec["tokens"].tolist() == plain[0, p.shape[1]:].tolist()
        assert [int(s.argmax()) for s in out.scores] == rec["tokens"].tolist()
        assert rec["member_tokens"].shape == (7, 3) and rec["masked_numbers"].shape == (7, 3) and rec["top_logprobs"].shape == (7, 8)
        assert lane.masked_numbers == [] and lane.engine._rec_buf is None      # as after the plain call; the ring is detached again
        # one image at a time on fresh lanes (one reference process per lane: its rng stream continues from image to image)
        solo = {}
        for lane_imgs in ([0, 4], [1, 5], [2], [3]):
            s = m.spawn_lane()
            for i in lane_imgs:
                o = s.generate(input_ids=imgs[i][0], pixel_values=imgs[i][1], max_new_tokens=6, eos_token_id=[], return_dict_in_generate=True,
                               output_logits=True)
                solo[i] = (o.sequences.cpu(), o.dropout_record["raw"].cpu(), torch.cat(o.logits).cpu())
                assert o.scores is None
        pipe = GroupPipeline(m.spawn_lane(), lanes=2)
        batches = [[dict(input_ids=p, pixel_values=v) for p, v in imgs[2 * b:2 * b + 2]] for b in range(3)]
        got = [o for outs in pipe.run(batches, max_new_tokens=6, eos_token_id=[], return_dict_in_generate=True, output_logits=True) for o in outs]
        assert len(got) == 6
        for i, o in enumerate(got):
            assert torch.equal(o.sequences.cpu(), solo[i][0]), f"pipeline image {i}"
            assert torch.equal(o.dropout_record["raw"].cpu(), solo[i][1]), f"pipeline image {i}: record bytes"
            assert torch.equal(torch.cat(o.logits).cpu(), solo[i][2]), f"pipeline image {i}: score rows"
        lanes = [m.spawn_lane() for _ in range(3)]
        outs = generate_group(lanes, [dict(input_ids=p, pixel_values=v) for p, v in imgs[:3]], max_new_tokens=6, eos_token_id=[],
                              return_dict_in_generate=True, output_logits=True)
        for i, o in zip((0, 1, 2), outs):
            assert torch.equal(o.sequences.cpu(), solo[i][0]) and torch.equal(o.dropout_record["raw"].cpu(), solo[i][1]), f"group image {i}"
        # several questions about one image: with settings['reuse_image_prefix'] the second and third prompt keep the image prefix and
        # prefill only their own text (truncate + extend); their records start again at slot 0 and describe the same decode as a full
        # prefill of the same prompt.  The bound is not exact here because the comparison is with ANOTHER prefill form: truncate + extend and
        # a full prefill agree within fp32 rounding (tests/test_gpu_engine.py: 2e-5 of the largest logit), so the log-probabilities are held
        # to twice that; the byte-exact comparison of a reused prompt with its own fresh truncate + extend decode is
        # test_truncate_and_extend_start_again_at_slot_zero
        qs = [torch.tensor([[1, 17, 511, 45, 6, 7, 99]]), torch.tensor([[1, 17, 511, 88, 3]]), torch.tensor([[1, 17, 511, 9, 9, 9, 12, 40]])]
        kw = dict(pixel_values=imgs[0][1], max_new_tokens=4, eos_token_id=[], return_dict_in_generate=True, output_scores=True)
        full_lane = m.spawn_lane()
        full_lane.engine.rng.manual_seed(11)
        full = [full_lane.generate(input_ids=q, **kw) for q in qs]
        ddc.settings["reuse_image_prefix"] = True
        try:
            re_lane = m.spawn_lane()
            re_lane.engine.rng.manual_seed(11)
            reused = [re_lane.generate(input_ids=q, **kw) for q in qs]
        finally:
            ddc.settings.pop("reuse_image_prefix")
        for q, a, b in zip(qs, full, reused):
            assert torch.equal(a.sequences, b.sequences)
            ra, rb = a.dropout_record, b.dropout_record
            assert rb["tokens"].tolist() == b.sequences[0, q.shape[1]:].tolist() and len(b.scores) == 4
            assert int(rb["winner"][0]) == -1 and int(rb["K"][0]) == 0 and rb["K"][1:].tolist() == [3, 3, 3]
            tol = 2 * 2e-5 * float(torch.cat(a.scores).abs().max())
            assert float((ra["token_logprobs"] - rb["token_logprobs"]).abs().max()) <= tol
            assert float((ra["base_token_logprobs"] - rb["base_token_logprobs"]).abs().max()) <= tol
    finally:
        ddc.settings["voting_numbers"] = saved


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------
def test_tensor_parallel_ranks_and_phase_calls_refuse_a_record(E):
    eng, w = _small(E)
    emb = torch.randn(58, 256, generator=torch.Generator().manual_seed(3)).cuda()
    eng.attach_record(4)
    eng.prefill(emb, 4, 40)
    with pytest.raises(ValueError, match="generation record is attached"):
        eng.step_base([0.3, 0.5, 0.7])
    eng._last_K = 0
    with pytest.raises(ValueError, match="generation record is attached"):
        eng.step_members(0, 0)
    with pytest.raises(ValueError, match="generation record is attached"):
        eng.step_commit()
    eng.detach_record()
    eng.step_base([0.3, 0.5, 0.7])                   # without a record the phase calls work as before
    eng.step_members(0, 3)
    eng.step_commit()
    assert eng.n_tokens() == 2
    eng.close()
    grp = E.TensorParallelGroup(E.LMConfig(512, 512, 1280, 2, 4, 4, 128, 1e-5, 10000.0), 2, family=FAMILY_LLAVA, max_seq=192, max_visual=40, seed=77)
    with pytest.raises(ValueError, match="tensor-parallel shard"):
        grp.ranks[0].attach_record(4)
    grp.close()


# ---- record 0 of the first-token ensemble ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,K", [(FAMILY_LLAVA, 3), (FAMILY_NEXT, 4), (FAMILY_LLAVA, 8)])
def test_first_token_ensemble_writes_a_real_ensemble_record(E, family, K):
    """dd_lm_prefill_ensemble (the `# if True:` toggle, models/llava.py:336-337): record 0 is an ensemble record with K > 0.  The cases
    of tests/test_gpu_engine.py test_first_token_ensemble_toggle, against RefDecoder(first_step_ensemble=True).first_record."""
    rc = RefCfg(*SMALL)
    probs = [0.1 + 0.1 * i for i in range(K)]
    T0, s0, L, n_new, seed = 70, 3, 50, 5, 5
    w = random_weights(rc, 23, 0.05)
    eng = E.DropoutEngine(E.LMConfig(*SMALL), family=family, max_seq=T0 + n_new + 8, max_visual=L, seed=seed)
    eng.load_state_dict(w)
    emb = torch.randn(T0, rc.hidden_size, generator=torch.Generator().manual_seed(seed)) * 0.8
    ref = RefDecoder(family, rc, w, probs, seed=seed, first_step_ensemble=True)
    want = ref.generate(emb, s0, L, n_new)
    eng.attach_record(n_new, scores=True)
    eng.prefill(emb.cuda(), s0, L, first_step_ensemble=True, mprobs=probs)
    for s in range(n_new - 1):
        eng.decode_step(probs)
    assert eng.tokens() == want
    r = _cpu(eng.record())
    for i, sr in enumerate([ref.first_record] + ref.records):
        info = f"record {i}"
        assert r["tokens"][i] == sr.token and r["base_tokens"][i] == sr.base_argmax and r["winner"][i] == sr.winner and r["K"][i] == K, info
        assert r["member_tokens"][i].tolist() == sr.member_argmax and r["masked_numbers"][i].tolist() == sr.masked_numbers, info
        assert r["votes"][i] == sum(1 for a in sr.member_argmax if a == sr.member_argmax[sr.winner]), info
        for row, lg, key in ((r["scores"][i], sr.logits, "token_logprobs"), (None, sr.base_logits, "base_token_logprobs")):
            big = float(np.abs(np.asarray(lg, np.float64)).max())
            if row is not None:
                assert float(np.abs(row.astype(np.float64) - lg).max()) <= 1e-3 * big, info
            assert abs(float(r[key][i]) - float(_log_softmax64(lg)[sr.token])) <= 2e-3 * big, f"{info}: {key}"
    eng.close()


# ---- vocabulary sizes off the 256-column stride, larger logits --------------------------------------------------------------------------
@pytest.mark.parametrize("V", [32064, 1000])
def test_kernel_arithmetic_at_vocab_sizes_off_the_stride(E, V):
    """V = 32064 (the 7B vocabulary: 32064 % 256 = 64, the bound's own size) and V = 1000 (Vpad = 1008 != V, so the winner's row sits at
    winner * Vpad and the last quad is cut), with an lm_head scaled up so that the logits reach well into the |x| <= 32 the bound is
    stated for.  float64 recomputation from the recorded rows; K = 3 steps, so rows 1.. come from member_logits + winner * Vpad."""
    dims = (V, 256, 512, 2, 2, 2, 128, 1e-5, 10000.0)
    w = dict(random_weights(RefCfg(*dims), 17, 0.05))
    w["lm_head.weight"] = w["lm_head.weight"] * 6.0
    eng = E.DropoutEngine(E.LMConfig(*dims), family=FAMILY_LLAVA, max_seq=160, max_visual=40, seed=11)
    eng.load_state_dict(w)
    emb = torch.randn(58, 256, generator=torch.Generator().manual_seed(3)).cuda()
    n_new = 10
    eng.attach_record(n_new, scores=True)
    eng.prefill(emb, 4, 40)
    for s in range(n_new - 1):
        eng.decode_step([0.3, 0.5, 0.7])
    toks = eng.tokens()
    np.testing.assert_array_equal(eng.logits(), eng.record()["scores"][n_new - 1].cpu().numpy())       # the row recorded IS the winner's row
    r = _cpu(eng.record())
    assert r["tokens"].tolist() == toks and r["scores"].shape == (n_new, V)
    worst = {"lse": 0.0, "logprob": 0.0, "base_logprob_vs_own_row": 0.0, "entropy": 0.0, "absmax": 0.0}
    for i in range(n_new):
        row = r["scores"][i]
        x = row.astype(np.float64)
        worst["absmax"] = max(worst["absmax"], float(np.abs(x).max()))
        ls = _log_softmax64(x)
        tok = int(r["tokens"][i])
        assert r["top_ids"][i].tolist() == _top8(row).tolist(), f"record {i}: top-8 ids"
        np.testing.assert_array_equal(r["top_logits"][i], row[r["top_ids"][i]])
        assert r["max_logit"][i] == row.max() and tok == int(np.argmax(row))
        worst["lse"] = max(worst["lse"], abs(float(r["lse"][i]) - float(x[tok] - ls[tok])))
        worst["logprob"] = max(worst["logprob"], abs(float(r["token_logprobs"][i]) - float(ls[tok])))
        worst["entropy"] = max(worst["entropy"], abs(float(r["entropy"][i]) - float(-(np.exp(ls) * ls).sum())))
        if i == 0:                                   # record 0: the un-masked row is the recorded row
            worst["base_logprob_vs_own_row"] = abs(float(r["base_token_logprobs"][0]) - float(ls[tok]))
    warnings.warn(f"record kernel vs float64 of its own rows (V={V}, max |logit| {worst['absmax']:.3g}): max abs error lse {worst['lse']:.3g}, "
                  f"logprob {worst['logprob']:.3g}, entropy {worst['entropy']:.3g}, base logprob (record 0) {worst['base_logprob_vs_own_row']:.3g}")
    assert 4 <= worst["absmax"] <= 32, "the constructed logits left the range the bound is stated for"
    assert worst["lse"] <= 1e-5 and worst["logprob"] <= 1e-5 and worst["base_logprob_vs_own_row"] <= 1e-5
    assert worst["entropy"] <= 1e-5 * math.log(V)
    eng.close()
