"""The lm_head GEMM and its fused scorer statistics through the large prefill block, against the ORACLE.

From 1024 selected rows on (a visual span of 1023 tokens or more + the last position; LLaVA-NeXT's spans have 2928) `prefill_head`
(csrc/dd_engine.hip) runs the lm_head through the large block of csrc/dd_prefill.hip instead of k_gemm, and that one launch also carries
what no layer GEMM has: the `n_valid` column clip of a vocabulary that is no multiple of 16, accumulator tiles past the last weight
tile (`wv[j] == false`: weight-scale and bias indices forced to tile 0, values that must enter no statistic), and the softmax block
statistics {max, sum exp} per 64 columns that the uncertainty scorer consumes (`rowstat`, `cb < rowstat_ld`).  A wrong statistic
in a partly valid block moves the uncertainties, hence every mask — only for long spans.  The vocabulary sizes put the production edges
onto a small model (d = 256, d_ff = 512, two layers, two heads of 128):

  V = 1344   84 tiles = 2 x 32 + 20: the tile residue of 32064 (2004 = 62 x 32 + 20) — a last 512-column block with 20 live tiles
  V = 1003   Vpad = 1008, 63 tiles: the last tile has 11 valid columns, the last 64-column statistics block 43, the last wave one
             dead tile (InstructBLIP-Vicuna's 32001 is no multiple of 16 either)
  V = 528    33 tiles: the second column block has ONE live tile and three idle waves

and L = 1100 (1101 rows: a partial row block in every form) / L = 1023 (1024 rows: the threshold itself), bf16 and fp8 weights (fp8
brings `wscale` into the dead tiles' indexing; the oracle then runs on the dequantised weights).  Every form — tuning key 20 = 1
(k_gemm_dma, 160 or 128 rows per launch), 0 (k_gemm_big), 8, 10 (k_gemm_dma<.., 8 / 10>), and key 16 = 0 (k_gemm<.., 4, 4> with its own
statistics path) — must leave the same bits, and the default form is compared with `RefDecoder` by tests/lane_check.py's rules: all L
rows of image logits and the last row within 1e-3 of max |logit|, the uncertainties within rtol 5e-3, top-k ids exact except at rows
whose oracle boundary gap is under 1e-3 (reported), tokens / keep sets / mask flags / member ids of three steps exact except at a
near-tie of the element that differs (reported).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.decode_ref import FAMILY_LLAVA, RefDecoder
from oracle.lm_ref import LMConfig as RefCfg, random_weights

from lane_check import LaneCheck, report          # tests/lane_check.py

PROBS = [0.3, 0.5, 0.7]
STEPS = 3
FORMS = ((1024, 1), (1024, 0), (1024, 8), (1024, 10), (0, 1))      # (key 16, key 20); the first is the default


@pytest.fixture(scope="module")
def E():
    from dropoutdecoding_amd import build
    build.build()
    from dropoutdecoding_amd import lm
    return lm


def _record(e):
    u = e.vision_uncert_dict()
    vals, ids = e.topk()
    return [e.image_logits().copy(), e.logits().copy(), e.kv_sums().copy(), u["epis_uncert_per_token"].copy(), u["alea_uncert_per_token"].copy(),
            u["variance_per_token"].copy(), np.concatenate([u["variance"], u["epis_uncert"], u["alea_uncert"]]), vals.copy(), np.asarray(ids).copy()]


ITEMS = ("image logits", "last-row logits", "kv sums", "epistemic", "aleatoric", "variance", "scalars", "top-k values", "top-k ids")


@pytest.mark.parametrize("wfmt", ["bf16", "fp8"])
@pytest.mark.parametrize("V", [1344, 1003, 528])
@pytest.mark.parametrize("L", [1100, 1023])
def test_lm_head_through_the_large_block_vs_oracle(E, L, V, wfmt):
    from dropoutdecoding_amd import _lib
    from dropoutdecoding_amd.lm import dequantize_fp8, quantize_fp8
    lib = _lib.load()
    dims = (V, 256, 512, 2, 2, 2, 128, 1e-5, 10000.0)
    rc, cfg = RefCfg(*dims), E.LMConfig(*dims)
    w = random_weights(rc, 91, 0.05)
    T0, s0 = L + 10, 4
    x = torch.randn(T0, 256, generator=torch.Generator().manual_seed(17)) * 0.8
    wo = w if wfmt != "fp8" else {k: (dequantize_fp8(*quantize_fp8(v)) if v.dim() == 2 and "embed_tokens" not in k else v) for k, v in w.items()}
    ref = RefDecoder(FAMILY_LLAVA, rc, wo, PROBS, seed=3)
    ref.tokens_out = ref.generate(x, s0, L, STEPS + 1)
    e = E.DropoutEngine(cfg, family=FAMILY_LLAVA, max_seq=T0 + 64, max_visual=L, seed=3, weight_format=wfmt)
    e.load_state_dict(w)
    what = f"lm_head through the large block, L = {L}, V = {V}, {wfmt}"
    check = LaneCheck(what, e, ref, PROBS)
    outs = []
    xd = x.cuda()
    try:
        for fi, (big, dma) in enumerate(FORMS):
            lib.dd_set_tuning(16, big)
            lib.dd_set_tuning(20, dma)
            e.rng.manual_seed(3)
            e.prefill(xd, s0, L)
            e.set_eos([])
            if fi == 0:
                check.prefill()
            rec = _record(e)
            for s in range(STEPS):
                e.decode_step(PROBS)
                st = e.last_step()
                rec += [e.base_logits().copy(), e.logits().copy(), st["drop"].copy(), st["keep"].copy(), st["member_argmax"].copy()]
                if fi == 0:
                    check.step(s)
            rec.append(np.asarray(e.tokens()))
            if fi == 0:
                check.tokens()
            outs.append(rec)
    finally:
        lib.dd_set_tuning(15, 1)
        lib.dd_set_tuning(16, 1024)
        lib.dd_set_tuning(20, 1)
    # what the engine holds beyond the valid columns never reaches a reader: image_logits() has V columns of the Vpad-wide rows
    assert outs[0][0].shape == (L, V)
    for (big, dma), o in zip(FORMS[1:], outs[1:]):
        for j, (a, b) in enumerate(zip(o, outs[0])):
            name = ITEMS[j] if j < len(ITEMS) else ("tokens" if j == len(o) - 1 else f"step {(j - len(ITEMS)) // 5} item {(j - len(ITEMS)) % 5}")
            np.testing.assert_array_equal(a, b, err_msg=f"{what}: key 16 = {big}, key 20 = {dma} vs the default form: {name}")
    report([check], what, max_gone=1)
    e.close()
