"""The 7B-shape kernel instantiations against the ORACLE (not against each other).

The nine-plane / rider / half-plane / fp8 slice kernels that carry the headline exist only for K = 4096 / 11008 / 14336
(csrc/dd_gemv.hip try_slices*: `spw == 16 || 43 || 56`); tests/test_gpu_rider.py, test_gpu_half_planes.py and
test_gpu_gemv_slices.py compare those forms bit for bit with each other and with a sequence decoded alone.  This file
anchors them to the reference: two-layer models with the 7B widths (d = 4096, d_ff = 11008 / 14336, 32 heads, MHA / GQA 4,
V = 2048) carry seeded `random_weights` through `load_state_dict`, and EVERY lane is compared with its own `RefDecoder`
(oracle/decode_ref.py — the restatement of the member loop models/llava.py:292-376, llavanext.py:490-600) step by step:

  token ids, keep sets, mask flags, masked counts, member argmax ids, winner   exact
  winner's logits, un-masked logits                                            <= 1e-3 of max |logit| (north star)

A discrete result may only differ where the oracle itself puts the decision AT THE ELEMENT THAT DIFFERS inside the logits tolerance
(tests/lane_check.py states the rule per kind of result): a keep-set row whose top-k ids differ at a boundary gap < 1e-3, or else a
top-1 minus top-2 of the un-masked logits < 1e-3 of max |logit|; at every (member, token) whose mask flag differs, a uniform closer to
its drop probability than the two sides' fp32 uncertainties move that probability (at least the 1e-5 of
test_mid_scale_llava_shapes_vs_oracle; InstructBLIP: that token's uncertainty against that member's quantile threshold); for every
member whose argmax id differs, that member's own top-1 minus top-2 < 1e-3.  Such a lane leaves the comparison from that step on; the
test prints it, emits it as a warning (so that a `pytest -q` log carries it) and fails if more than one lane in eight does.  (The
streams are seeded, so a given tree either has such a flip or not — no flake.)

The batched prefill (dd_lm_prefill_group: >= 1024 rows, the large-block GEMM in each of its forms) is anchored here too:
test_batched_prefill_7b_widths_every_form_every_lane_vs_oracle.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.decode_ref import FAMILY_IBLIP, FAMILY_LLAVA, FAMILY_NEXT, RefDecoder
from oracle.lm_ref import LMConfig as RefCfg, random_weights

from lane_check import TOL, LaneCheck, report as _report          # tests/lane_check.py

K8 = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
K4 = [0.1, 0.3, 0.5, 0.7]             # the reference's shipped LLaVA-1.5 list (chair_test/chair_test.py:170)
STD = 0.012                           # d = 4096: q.k / sqrt(128) of a few units, logits of order one


@pytest.fixture(scope="module")
def E():
    from dropoutdecoding_amd import build
    build.build()
    from dropoutdecoding_amd import lm
    return lm


@pytest.fixture(scope="module")
def llama_w():
    dims = (2048, 4096, 11008, 2, 32, 32, 128, 1e-5, 10000.0)
    return dims, random_weights(RefCfg(*dims), 61, STD)


@pytest.fixture(scope="module")
def mistral_w():
    dims = (2048, 4096, 14336, 2, 32, 8, 128, 1e-5, 1000000.0)
    return dims, random_weights(RefCfg(*dims), 63, STD)


def _oracle_lanes(family, rc, w, probs, embs, spans, n_new, seed0=50):
    import time
    t0 = time.time()
    refs = []
    for i, (emb, (s0, L)) in enumerate(zip(embs, spans)):
        r = RefDecoder(family, rc, w, probs, seed=seed0 + i)
        r.tokens_out = r.generate(emb, s0, L, n_new)
        refs.append(r)
    print(f"\n[oracle: {len(refs)} lanes x {n_new} tokens in {time.time() - t0:.0f} s]", end="")
    return refs


def _lanes(E, cfg, n, family, max_visual, max_seq=None, **kw):
    import time
    t0 = time.time()
    engines = []
    for i in range(n):
        engines.append(E.DropoutEngine(cfg, family=family, max_seq=max_seq or max_visual + 96, max_visual=max_visual, seed=50 + i, kv_format="fp16",
                                       share_weights_with=engines[0] if engines else None, **kw))
    print(f"\n[{n} engines created in {time.time() - t0:.0f} s]", end="")
    return engines


def _inputs(n, d, L, seed):
    gen = torch.Generator().manual_seed(seed)
    T0s = [L + 6 + (i % 5) for i in range(n)]
    embs = [torch.randn(T0, d, generator=gen) * 0.5 for T0 in T0s]
    spans = [(2 + (i % 3), L) for i in range(n)]
    return embs, spans


def _group_vs_oracle(E, engines, refs, embs, spans, probs, steps, what):
    import time
    t0 = time.time()
    for i, (e, emb, (s0, L)) in enumerate(zip(engines, embs, spans)):
        e.rng.manual_seed(50 + i)
        e.prefill(emb.cuda(), s0, L)
        e.set_eos([])
    checks = [LaneCheck(f"{what}, lane {i}", e, r, probs) for i, (e, r) in enumerate(zip(engines, refs))]
    for c in checks:
        c.prefill()
    grp = E.EngineGroup(engines)
    for s in range(steps):
        grp.decode_step(probs)
        for c in checks:
            c.step(s)
    for c in checks:
        c.tokens()
    print(f"\n[engine side: {len(engines)} lanes, prefill + {steps} group steps + comparisons in {time.time() - t0:.0f} s]", end="")
    _report(checks, what)


def _solo_vs_oracle(e, ref, emb, span, probs, steps, seed, mode, what):
    e.set_speculation(mode)
    e.rng.manual_seed(seed)
    e.prefill(emb.cuda(), *span)
    e.set_eos([])
    c = LaneCheck(what, e, ref, probs)
    c.prefill()
    for s in range(steps):
        e.decode_step(probs)
        c.step(s)
    c.tokens()
    e.set_speculation("default")
    assert c.live, c.excuse
    return c.worst


def test_rider_step_llama7b_shapes_every_lane_vs_oracle(E, llama_w):
    """(a) 16 lanes, K = 8, the rider form (72-row nine-plane kernels: K = 4096 single slices, K = 11008 `spw == 43`), then two of
    the lanes alone through the 8-row step and the speculative 16-row step.  The span crosses a 64-key attention tile."""
    dims, w = llama_w
    d = dims[1]
    rc, cfg = RefCfg(*dims), E.LMConfig(*dims)
    L, n, steps = 72, 16, 4
    embs, spans = _inputs(n, d, L, 9)
    refs = _oracle_lanes(FAMILY_LLAVA, rc, w, K8, embs, spans, steps + 1)
    engines = _lanes(E, cfg, n, FAMILY_LLAVA, L)
    engines[0].load_state_dict(w)
    _group_vs_oracle(E, engines, refs, embs, spans, K8, steps, "llama-7b shapes, 16 lanes K = 8 (rider form)")
    for li, mode in ((0, "never"), (9, "always")):
        worst = _solo_vs_oracle(engines[li], refs[li], embs[li], spans[li], K8, steps, 50 + li, mode,
                                f"llama-7b shapes, lane {li} alone (speculation {mode})")
        print(f"  lane {li} alone, speculation {mode}: worst logits error {worst:.2e}")
    for e in reversed(engines):
        e.close()


def test_half_plane_rider_k4_llama7b_shapes_every_lane_vs_oracle(E, llama_w):
    """(b) 28 lanes, K = 4: two sequences per operand plane, groups of fourteen in the rider form (seven half planes + two riding
    planes) — BASELINE config 2's step."""
    dims, w = llama_w
    d = dims[1]
    rc, cfg = RefCfg(*dims), E.LMConfig(*dims)
    L, n, steps = 40, 28, 3
    embs, spans = _inputs(n, d, L, 10)
    refs = _oracle_lanes(FAMILY_LLAVA, rc, w, K4, embs, spans, steps + 1)
    engines = _lanes(E, cfg, n, FAMILY_LLAVA, L)
    engines[0].load_state_dict(w)
    _group_vs_oracle(E, engines, refs, embs, spans, K4, steps, "llama-7b shapes, 28 lanes K = 4 (half-plane rider form)")
    for e in reversed(engines):
        e.close()


def test_rider_step_mistral7b_fp8_every_lane_vs_oracle(E, mistral_w):
    """(c) BASELINE config 5's weight format at its widths: d_ff = 14336, GQA 4, fp8 e4m3fn tiles + row scales; nine-plane fp8 slice
    kernels and the chunked K = 14336 kernel.  The oracle runs on the DEQUANTISED weights (scale * q in fp32: the arithmetic the
    kernels restate exactly), LLaVA-NeXT rule (masks reset every step).  Then one lane alone: 8-row fp8 kernels, both step forms."""
    from dropoutdecoding_amd.lm import dequantize_fp8, quantize_fp8
    dims, w = mistral_w
    d = dims[1]
    rc, cfg = RefCfg(*dims), E.LMConfig(*dims)
    wq = {k: (dequantize_fp8(*quantize_fp8(v)) if v.dim() == 2 and "embed_tokens" not in k else v) for k, v in w.items()}
    L, n, steps = 40, 16, 3
    embs, spans = _inputs(n, d, L, 11)
    refs = _oracle_lanes(FAMILY_NEXT, rc, wq, K8, embs, spans, steps + 1)
    del wq
    engines = _lanes(E, cfg, n, FAMILY_NEXT, L, weight_format="fp8")
    engines[0].load_state_dict(w)
    _group_vs_oracle(E, engines, refs, embs, spans, K8, steps, "mistral-7b shapes fp8, 16 lanes K = 8 (rider form)")
    for li, mode in ((12, "always"),):          # (the two-sweep 8-row fp8 step: test_fp8_weight_storage_next_family's kernels, K = 14336 here)
        worst = _solo_vs_oracle(engines[li], refs[li], embs[li], spans[li], K8, steps, 50 + li, mode,
                                f"mistral-7b shapes fp8, lane {li} alone (speculation {mode})")
        print(f"  lane {li} alone, speculation {mode}: worst logits error {worst:.2e}")
    for e in reversed(engines):
        e.close()


def test_solo_mistral7b_bf16_both_step_forms_vs_oracle(E, mistral_w):
    """(d) the 16-bit kernels at d_ff = 14336 (`spw == 56`), GQA 4: one sequence through the two-sweep 8-row step and the speculative
    16-row step, and 16 lanes in the rider form, each lane against its oracle."""
    dims, w = mistral_w
    d = dims[1]
    rc, cfg = RefCfg(*dims), E.LMConfig(*dims)
    L, n, steps = 72, 16, 3
    embs, spans = _inputs(n, d, L, 12)
    refs = _oracle_lanes(FAMILY_NEXT, rc, w, K8, embs, spans, steps + 1)
    engines = _lanes(E, cfg, n, FAMILY_NEXT, L)
    engines[0].load_state_dict(w)
    _group_vs_oracle(E, engines, refs, embs, spans, K8, steps, "mistral-7b shapes bf16, 16 lanes K = 8 (rider form)")
    for li, mode in ((0, "never"),):
        worst = _solo_vs_oracle(engines[li], refs[li], embs[li], spans[li], K8, steps, 50 + li, mode,
                                f"mistral-7b shapes bf16, lane {li} alone (speculation {mode})")
        print(f"  lane {li} alone, speculation {mode}: worst logits error {worst:.2e}")
    for e in reversed(engines):
        e.close()


def test_rider_step_instructblip_rule_llama7b_shapes_every_lane_vs_oracle(E, llama_w):
    """(e) BASELINE config 4's rule at its language model's widths (Vicuna-7B = LLaMA-7B shapes): quantile masks (no random draws), the vote on the
    argmax of the final hidden state, the last member's zeros leaking into the next un-masked row — 16 lanes in the rider form, each against its own
    oracle, then one lane alone.  32 visual tokens at the start of the sequence, as the Q-Former delivers them."""
    dims, w = llama_w
    d = dims[1]
    rc, cfg = RefCfg(*dims), E.LMConfig(*dims)
    L, n, steps = 32, 16, 3
    gen = torch.Generator().manual_seed(13)
    embs = [torch.randn(L + 8 + (i % 5), d, generator=gen) * 0.5 for i in range(n)]
    spans = [(0, L)] * n
    refs = _oracle_lanes(FAMILY_IBLIP, rc, w, K8, embs, spans, steps + 1)
    engines = _lanes(E, cfg, n, FAMILY_IBLIP, L)
    engines[0].load_state_dict(w)
    _group_vs_oracle(E, engines, refs, embs, spans, K8, steps, "llama-7b shapes, InstructBLIP rule, 16 lanes K = 8 (rider form)")
    worst = _solo_vs_oracle(engines[7], refs[7], embs[7], spans[7], K8, steps, 57, "never", "llama-7b shapes, InstructBLIP rule, lane 7 alone")
    print(f"  lane 7 alone: worst logits error {worst:.2e}")
    for e in reversed(engines):
        e.close()


def _lane_record(e):
    return [e.image_logits().copy(), e.logits().copy(), e.kv_sums().copy(), e.vision_uncert_dict()["epis_uncert_per_token"].copy(),
            np.asarray(e.topk()[1]).copy()]


@pytest.mark.parametrize("which,wfmt", [("llama_w", "bf16"), ("mistral_w", "bf16"), ("mistral_w", "fp8")])
def test_batched_prefill_7b_widths_every_form_every_lane_vs_oracle(E, request, which, wfmt):
    """(f) dd_lm_prefill_group at the 7B widths: nine prompts of 103 .. 250 positions laid back to back as ONE matrix of 9 x 256 = 2304 rows, which
    every GEMM of the layers (K = 4096 / 11008 / 14336: 128 / 344 / 448 k-steps; EPI_QKV, EPI_RESID, EPI_SILU; bf16 and the fp8 scales) runs
    through the large block — in each of its forms, tuning key 20 = 1 (LDS-DMA, 160 or 128 rows per launch), 0 (k_gemm_big), 8 and 10
    (k_gemm_dma<.., 8 / 10> forced).  256 is no multiple of 160, so the 160-row blocks straddle sequences, and 2304 = 14 x 160 + 64 leaves a
    partial last block; the spans start at different offsets and cross 64-key tiles.  After each prefill two group steps read the KV cache
    that the batched QKV epilogue wrote per sequence.  The four forms and one prefill() per lane (under 1024 rows: k_gemm) must leave the same
    bits — image logits, last-row logits, cache sums, uncertainties, top-k ids, both steps' logits, tokens — and the default form's run is
    compared lane by lane with each lane's own oracle (fp8: the oracle on the dequantised weights)."""
    import time
    from dropoutdecoding_amd import _lib
    from dropoutdecoding_amd.lm import dequantize_fp8, quantize_fp8
    lib = _lib.load()
    dims, w = request.getfixturevalue(which)
    d = dims[1]
    rc, cfg = RefCfg(*dims), E.LMConfig(*dims)
    family, probs = (FAMILY_LLAVA, K4) if which == "llama_w" else (FAMILY_NEXT, K8)
    T0s = [103, 250, 137, 199, 129, 241, 160, 117, 222]              # max 250 -> 256 rows per sequence; 137, 199, ... in (128, 256]
    spans = [(2, 72), (30, 80), (60, 40), (5, 96), (50, 64), (100, 90), (0, 48), (20, 50), (120, 64)]   # (60, 40), (50, 64), (20, 50): across key 64
    n, steps = len(T0s), 2
    gen = torch.Generator().manual_seed(14)
    embs = [torch.randn(T0, d, generator=gen) * 0.5 for T0 in T0s]
    wo = w if wfmt != "fp8" else {k: (dequantize_fp8(*quantize_fp8(v)) if v.dim() == 2 and "embed_tokens" not in k else v) for k, v in w.items()}
    refs = _oracle_lanes(family, rc, wo, probs, embs, spans, steps + 1)
    del wo
    engines = _lanes(E, cfg, n, family, 96, max_seq=320, weight_format=wfmt)
    engines[0].load_state_dict(w)
    xs = [x.cuda() for x in embs]
    grp = E.EngineGroup(engines)
    what = f"{which[:-2]}-7b shapes {wfmt}, batched prefill of {n} lanes ({n} x 256 rows)"
    checks = [LaneCheck(f"{what}, lane {i}", e, r, probs) for i, (e, r) in enumerate(zip(engines, refs))]

    def run(form):
        """form: key 20's value, or None = one prefill() per lane"""
        for i, e in enumerate(engines):
            e.rng.manual_seed(50 + i)
        if form is None:
            for e, x, (s0, L) in zip(engines, xs, spans):
                e.prefill(x, s0, L)
        else:
            lib.dd_set_tuning(20, form)
            E.prefill_group(engines, xs, spans)
        for e in engines:
            e.set_eos([])
        if form == 1:
            for c in checks:
                c.prefill()
        rec = [_lane_record(e) for e in engines]
        for s in range(steps):
            grp.decode_step(probs)
            for e, r in zip(engines, rec):
                r += [e.base_logits().copy(), e.logits().copy(), e.last_step()["drop"].copy()]
            if form == 1:
                for c in checks:
                    c.step(s)
        for e, r in zip(engines, rec):
            r.append(np.asarray(e.tokens()))
        if form == 1:
            for c in checks:
                c.tokens()
        return rec

    t0 = time.time()
    try:
        outs = {form: run(form) for form in (1, 0, 8, 10)}
    finally:
        lib.dd_set_tuning(15, 1)
        lib.dd_set_tuning(16, 1024)
        lib.dd_set_tuning(20, 1)
    outs["prefill() per lane"] = run(None)
    print(f"\n[engine side: {n} lanes, 5 x (prefill + {steps} group steps) + comparisons in {time.time() - t0:.0f} s]", end="")
    for form, recs in outs.items():
        for i, (got, want) in enumerate(zip(recs, outs[1])):
            for j, (a, b) in enumerate(zip(got, want)):
                np.testing.assert_array_equal(a, b, err_msg=f"{what}: form {form} vs form 1, lane {i}, item {j} "
                                                            "(0 image logits, 1 last logits, 2 kv sums, 3 epi, 4 top-k ids, then per step "
                                                            "un-masked logits, logits, drop flags; last: tokens)")
    _report(checks, what)
    for e in reversed(engines):
        e.close()
