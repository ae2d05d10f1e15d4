"""MXFP4 weight storage (dd_lm_config.weight_format 3): e2m1 elements + one e8m0 scale per 32 k, expanded exactly to bf16 in the
kernels.  The engine computes "fp32 activations x the dequantised matrix", so the oracle runs on the dequantised weights and the
usual tolerances apply (DESIGN.md "Numerics"): tokens, masks, member argmax, winner exact; logits 1e-3 of the largest |logit|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lane_check import TOL, LaneCheck, mask_distance, report, top_gap
from oracle.decode_ref import FAMILY_LLAVA, FAMILY_NEXT, RefDecoder
from oracle.lm_ref import LMConfig as RefCfg, random_weights


@pytest.fixture(scope="module")
def E():
    from dropoutdecoding_amd import build
    build.build()
    from dropoutdecoding_amd import lm
    return lm


def _cfg(E, rc):
    return E.LMConfig(rc.vocab_size, rc.hidden_size, rc.intermediate_size, rc.num_layers, rc.num_heads, rc.num_kv_heads, rc.head_dim,
                      rc.rms_eps, rc.rope_theta)


def _dequantised(E, w):
    """the state dict an MXFP4 engine holds: matrices through quantize -> dequantize, embedding and norm vectors as they are"""
    return {k: (E.dequantize_mxfp4(*E.quantize_mxfp4(v)) if v.dim() == 2 and "embed_tokens" not in k else v) for k, v in w.items()}


def _load_raw(eng, E, tid, layer, q, s, rows, cols):
    from dropoutdecoding_amd import _lib
    _lib.check(eng.lib.dd_lm_load_tensor_mxfp4(eng._h, tid, layer, q.data_ptr(), s.data_ptr(), rows, cols, 0), "dd_lm_load_tensor_mxfp4")


def test_every_code_position_and_scale(E):
    """All 16 e2m1 codes on the diagonal of a 256 x 256 lm_head: both nibbles, every k of two 128-k loads, every lane, block scales
    2^-20 .. 2^20 and the two ends of the accepted range — through the expansion for the prefill GEMM and through the 8-row GEMV's
    in-register path (the un-masked row of one ensemble step).  logits[n] = W[n, n] * hidden[n]: one product per output, the slack is
    the hi/lo split of the activation (tests/test_gpu_engine.py test_fp8_conversion_is_ocp_e4m3fn's rtol).
    The engine keeps the hidden state behind the prefill's logits (DD_GET_HIDDEN) but not the one behind a step's un-masked logits, so
    the step's hidden state is read through an identity head first: code 2 (= 1.0) with scale byte 127 on the diagonal gives
    logits = hi + lo of the hidden state (2^-17 of slack, inside the rtol).  Every row of the embedding table is the same vector, so the
    step's input — the token the head under test picked — does not change that hidden state; the other kernels are deterministic."""
    V, d = 256, 256
    rc = RefCfg(V, d, 256, 1, 2, 2, 128, 1e-5, 10000.0)
    w = random_weights(rc, 1, 0.05)
    w["model.embed_tokens.weight"] = w["model.embed_tokens.weight"][:1].repeat(V, 1)
    eng = E.DropoutEngine(_cfg(E, rc), family=FAMILY_LLAVA, max_seq=64, max_visual=8, weight_format="mxfp4")
    eng.load_state_dict(w)
    n = torch.arange(V)
    probs = [0.3, 0.5, 0.7]
    x = torch.randn(10, d, generator=torch.Generator().manual_seed(5)).cuda()

    def head(c, scale):
        codes = torch.zeros(V, d, dtype=torch.uint8)
        codes[n, n] = c
        q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
        _load_raw(eng, E, E.T_LM_HEAD, 0, q, scale, V, d)
        return q, E.dequantize_mxfp4(q, scale)[n, n].numpy()

    _, one = head(2, torch.full((V, d // 32), 127, dtype=torch.uint8))
    assert (one == 1.0).all()
    eng.prefill(x, 1, 8)
    np.testing.assert_allclose(eng.logits(), eng.hidden(), rtol=2e-5, atol=0, err_msg="identity head")
    eng.decode_step(probs)
    hid_step = eng.base_logits().copy()                     # the final-normed hidden state of the step's un-masked row
    assert np.isfinite(hid_step).all() and np.count_nonzero(hid_step) == d

    scale = (127 + ((torch.arange(d // 32)[None, :] + n[:, None]) % 41 - 20)).to(torch.uint8)    # (row n, block b); b = n // 32 on the diagonal
    scale[[3, 100]] = 7
    scale[[50, 200]] = 247
    for c in range(16):
        q, diag = head(c, scale)
        assert np.count_nonzero(diag) == (0 if c in (0, 8) else V)
        eng.prefill(x, 1, 8)
        np.testing.assert_allclose(eng.logits(), diag * eng.hidden(), rtol=2e-4, atol=0, err_msg=f"code {c}: prefill GEMM")
        eng.decode_step(probs)
        np.testing.assert_allclose(eng.base_logits(), diag * hid_step, rtol=2e-4, atol=0, err_msg=f"code {c}: 8-row GEMV")
    for bad in (255, 3):
        s2 = scale.clone()
        s2[77, 5] = bad
        with pytest.raises(ValueError):
            _load_raw(eng, E, E.T_LM_HEAD, 0, q, s2, V, d)
    eng.close()


def test_prefill_is_the_bf16_engines_bit_for_bit(E):
    """The expansion is exact and the prefill GEMM is the same code: an MXFP4 engine and a bf16 engine that holds the dequantised
    matrices produce the same bits — a 70-row prefill and a 40-row extension (the GEMM path, > 32 rows)."""
    rc = RefCfg(512, 512, 768, 2, 4, 4, 128, 1e-5, 10000.0)
    w = random_weights(rc, 40, 0.05)
    a = E.DropoutEngine(_cfg(E, rc), family=FAMILY_LLAVA, max_seq=192, max_visual=48, weight_format="mxfp4")
    b = E.DropoutEngine(_cfg(E, rc), family=FAMILY_LLAVA, max_seq=192, max_visual=48, weight_format="bf16")
    a.load_state_dict(w)
    b.load_state_dict(_dequantised(E, w))
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(70, 512, generator=g) * 0.8).cuda()
    tail = (torch.randn(40, 512, generator=g) * 0.8).cuda()

    def same(what):
        np.testing.assert_array_equal(a.logits(), b.logits(), err_msg=what)
        np.testing.assert_array_equal(a.kv_sums(), b.kv_sums(), err_msg=what)
        assert a.tokens() == b.tokens(), what
    a.prefill(x, 5, 48)
    b.prefill(x, 5, 48)
    same("prefill")
    np.testing.assert_array_equal(a.image_logits(), b.image_logits())
    ua, ub = a.vision_uncert_dict(), b.vision_uncert_dict()
    for k in ua:
        np.testing.assert_array_equal(ua[k], ub[k], err_msg=k)
    np.testing.assert_array_equal(a.topk()[1], b.topk()[1])
    np.testing.assert_array_equal(a.topk()[0], b.topk()[0])
    for e in (a, b):
        e.truncate(70)
        e.prefill_extend(tail)
    same("prefill_extend, 40 rows")
    a.close()
    b.close()


ORACLE_CASES = {
    "next": (FAMILY_NEXT, RefCfg(512, 512, 512, 2, 4, 2, 128, 1e-5, 1e6), 36, 7, 6, 4, [0.2, 0.4, 0.6, 0.8]),
    "llava": (FAMILY_LLAVA, RefCfg(512, 512, 768, 2, 4, 4, 128, 1e-5, 1e4), 40, 7, 5, 7, [0.3, 0.5, 0.7]),
}


@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_one_sequence_against_the_oracle(E, case):
    """70 prompt rows, a 48-token span, 7 new tokens, under both fixed speculation policies (identical results).  The oracle's smallest
    decision margins over these runs (member top-1 - top-2, un-masked, prefill, nearest uniform to its threshold) are 9.3e-3, 3.3e-3,
    7.5e-3, 1.7e-3 (next) and 9.3e-3, 2.7e-3, 6.0e-2, 2.3e-3 (llava): no near-tie excuse is needed; image rows do have top-k
    near-ties (5e-5 / 2e-4), which is what LaneCheck's topk_note rule covers — nothing else may take the lane out of the comparison."""
    family, rc, wseed, es, s0, seed, probs = ORACLE_CASES[case]
    w = random_weights(rc, wseed, 0.05)
    emb = torch.randn(70, 512, generator=torch.Generator().manual_seed(es)) * 0.8
    ref = RefDecoder(family, rc, _dequantised(E, w), probs, seed=seed)
    ref.tokens_out = ref.generate(emb, s0, 48, 7)
    runs = {}
    for mode in ("never", "always"):
        eng = E.DropoutEngine(_cfg(E, rc), family=family, max_seq=160, max_visual=48, seed=seed, weight_format="mxfp4")
        eng.load_state_dict(w)
        eng.set_speculation(mode)
        eng.prefill(emb.cuda(), s0, 48)
        c = LaneCheck(f"mxfp4 {case} (speculation {mode})", eng, ref, probs)
        c.prefill()
        rec = []
        for s in range(6):
            eng.decode_step(probs)
            c.step(s)
            st = eng.last_step()
            rec.append((st["drop"].copy(), st["member_argmax"].tolist(), st["winner"], eng.logits().copy(), eng.base_logits().copy()))
        c.tokens()
        assert c.live or (c.topk_note and "keep set" in c.excuse), c.excuse       # the only excuse: a keep set that felt a top-k near-tie of an image row
        report([c], f"mxfp4 {case}, speculation {mode}", max_gone=1)
        runs[mode] = (eng.tokens(), rec)
        eng.close()
    assert runs["never"][0] == runs["always"][0]
    for s, (x, y) in enumerate(zip(runs["never"][1], runs["always"][1])):
        np.testing.assert_array_equal(x[0], y[0], err_msg=f"step {s}")
        assert x[1] == y[1] and x[2] == y[2], s
        np.testing.assert_array_equal(x[3], y[3], err_msg=f"step {s}")
        np.testing.assert_array_equal(x[4], y[4], err_msg=f"step {s}")


def test_lanes_against_the_oracle(E):
    """11 lanes over one weight owner (16-row un-masked pass, 4 + 4 + 2 + 1 member sweeps through the grouped GEMV): every lane against
    its own reference process; at most one lane in eight (here: one) may leave at a near-tie of the oracle's own (tests/lane_check.py)."""
    family, rc, wseed, _, _, seed, probs = ORACLE_CASES["next"]
    w = random_weights(rc, wseed, 0.05)
    wq = _dequantised(E, w)
    shapes = [(60 + 5 * i, 3 + i % 4, 40) for i in range(11)]
    engs = []
    for i in range(len(shapes)):
        engs.append(E.DropoutEngine(_cfg(E, rc), family=family, max_seq=192, max_visual=40, seed=seed, weight_format="mxfp4",
                                    share_weights_with=engs[0] if engs else None))
    engs[0].load_state_dict(w)
    embs = [torch.randn(T0, 512, generator=torch.Generator().manual_seed(70 + i)) * 0.8 for i, (T0, _, _) in enumerate(shapes)]
    checks = []
    for i, (e, x, (T0, s0, L)) in enumerate(zip(engs, embs, shapes)):
        e.prefill(x.cuda(), s0, L)
        ref = RefDecoder(family, rc, wq, probs, seed=seed)
        ref.tokens_out = ref.generate(x, s0, L, 6)
        c = LaneCheck(f"lane {i}", e, ref, probs)
        c.prefill()
        checks.append(c)
    toks = E.EngineGroup(engs).generate(6, mprobs=probs)
    for i, c in enumerate(checks):
        want = c.ref.tokens_out
        if toks[i] == want:
            c.step(len(c.ref.records) - 1)                     # the last step's masks, member ids, winner and logits
            continue
        # the lane went another way at some step: a wrong result unless the ORACLE has a near-tie at that step (lane_check.py's kinds)
        first = next(s for s, (p, q) in enumerate(zip(toks[i], want)) if p != q)
        assert first >= 1, f"lane {i}: the prefill's token differs"
        r = c.ref.records[first - 1]
        if c.topk_note:
            c.live, c.excuse = False, f"lane {i}: token {first} differs ({c.topk_note})"
            continue
        d = float(mask_distance(r, c.ref, probs).min())
        if d < c.p_limit:
            c._excused(f"token {first} differs behind a mask decision", d, c.p_limit, first - 1)
        else:
            c._excused(f"token {first} differs", min([top_gap(r.base_logits)] + list(r.member_margin or [])), TOL, first - 1)
    report(checks, "mxfp4, 11 lanes")
    for e in reversed(engs):
        e.close()


def test_lanes_full_length_loops_equal_solo_runs(E):
    """d = 2048, d_ff = 5632: 16 and 44 loads of 128 k per tile row (44 = five rounds of the 8 waves + 4: the uneven tail), 5 lanes,
    synthetic weights: drop flags, logits and un-masked logits of three group steps, bit for bit against each lane alone."""
    probs = [0.2, 0.4, 0.6, 0.8]
    big = E.LMConfig(4099, 2048, 5632, 2, 16, 16, 128, 1e-5, 10000.0)
    shapes = [(70, 3, 60), (80, 5, 64), (66, 1, 60), (90, 9, 70), (75, 2, 64)]
    engs = []
    for i in range(len(shapes)):
        engs.append(E.DropoutEngine(big, family=FAMILY_LLAVA, max_seq=128, max_visual=70, seed=9, weight_format="mxfp4",
                                    share_weights_with=engs[0] if engs else None))
    engs[0].load_synthetic(3, 0.03)
    embs = [torch.randn(T0, 2048, generator=torch.Generator().manual_seed(90 + i)).cuda() for i, (T0, _, _) in enumerate(shapes)]
    for e, x, (T0, s0, L) in zip(engs, embs, shapes):
        e.prefill(x, s0, L)
    grp = E.EngineGroup(engs)
    rec = [[] for _ in engs]
    for s in range(3):
        grp.decode_step(probs)
        for i, e in enumerate(engs):
            rec[i].append((e.last_step()["drop"].copy(), e.logits().copy(), e.base_logits().copy()))
    toks = [e.tokens() for e in engs]
    assert all(np.isfinite(r[1]).all() and np.abs(r[1]).max() > 0 for lane in rec for r in lane)
    for i, (e, x, (T0, s0, L)) in enumerate(zip(engs, embs, shapes)):
        e.rng.manual_seed(9)
        e.prefill(x, s0, L)
        for s in range(3):
            e.decode_step(probs)
            np.testing.assert_array_equal(e.last_step()["drop"], rec[i][s][0])
            np.testing.assert_array_equal(e.logits(), rec[i][s][1], err_msg=f"lane {i} step {s}")
            np.testing.assert_array_equal(e.base_logits(), rec[i][s][2], err_msg=f"lane {i} step {s}")
        assert e.tokens() == toks[i]
    for e in reversed(engs):
        e.close()


def test_twenty_lanes_take_the_two_pass_fallback(E):
    """20 lanes, K = 3: sweeps of eight sequences are 64-row passes, which MXFP4 tiles run as two 32-row passes (ddk_gemv_groups:
    no 64-row kernel for this format); a lane of the last sweep decodes what it decodes alone."""
    probs = [0.3, 0.5, 0.7]
    rc = ORACLE_CASES["next"][1]
    shapes = [(50 + 3 * i, 2 + i % 3, 40) for i in range(20)]
    engs = []
    for i in range(len(shapes)):
        engs.append(E.DropoutEngine(_cfg(E, rc), family=FAMILY_NEXT, max_seq=160, max_visual=40, seed=4, weight_format="mxfp4",
                                    share_weights_with=engs[0] if engs else None))
    engs[0].load_state_dict(random_weights(rc, 36, 0.05))
    embs = [(torch.randn(T0, 512, generator=torch.Generator().manual_seed(30 + i)) * 0.8).cuda() for i, (T0, _, _) in enumerate(shapes)]
    for e, x, (T0, s0, L) in zip(engs, embs, shapes):
        e.prefill(x, s0, L)
    E.EngineGroup(engs).decode_step(probs)
    e, x, (T0, s0, L) = engs[17], embs[17], shapes[17]
    toks, logits, base = e.tokens(), e.logits().copy(), e.base_logits().copy()
    e.rng.manual_seed(4)
    e.prefill(x, s0, L)
    e.decode_step(probs)
    assert e.tokens() == toks
    np.testing.assert_array_equal(e.logits(), logits)
    np.testing.assert_array_equal(e.base_logits(), base)
    for e in reversed(engs):
        e.close()


def test_refusals(E):
    from dropoutdecoding_amd import _lib
    rc = RefCfg(512, 256, 512, 1, 2, 2, 128, 1e-5, 10000.0)
    w = random_weights(rc, 2, 0.05)
    with pytest.raises((ValueError, _lib.DDError)):
        E.DropoutEngine(_cfg(E, rc), family=FAMILY_LLAVA, max_seq=64, max_visual=8, weight_format="mxfp4", tp=(0, 2))
    mx = E.DropoutEngine(_cfg(E, rc), family=FAMILY_LLAVA, max_seq=64, max_visual=8, weight_format="mxfp4")
    bf = E.DropoutEngine(_cfg(E, rc), family=FAMILY_LLAVA, max_seq=64, max_visual=8, weight_format="bf16")
    wq = w["model.layers.0.self_attn.q_proj.weight"]
    with pytest.raises(ValueError):
        mx._load(E.T_WQ, 0, wq)                               # a bf16 matrix into an MXFP4 engine
    with pytest.raises(ValueError):
        mx._load_fp8(E.T_WQ, 0, wq)                           # the fp8 loader refuses it too
    with pytest.raises(ValueError):
        bf._load_mxfp4(E.T_WQ, 0, wq)                         # the MXFP4 loader on a bf16 engine
    with pytest.raises(ValueError):
        mx._load_mxfp4(E.T_ATTN_NORM, 0, torch.ones(256, 256))   # not a matrix id
    with pytest.raises(ValueError):
        mx._load_mxfp4(E.T_WQ, 0, wq[:, :128])                # wrong shape
    lane = E.DropoutEngine(_cfg(E, rc), family=FAMILY_LLAVA, max_seq=64, max_visual=8, weight_format="mxfp4", share_weights_with=mx)
    with pytest.raises(ValueError):
        lane._load_mxfp4(E.T_WQ, 0, wq)                       # a handle that borrows its weights
    mx._load(E.T_ATTN_NORM, 0, w["model.layers.0.input_layernorm.weight"])     # norm vectors stay 16-bit
    assert mx.algorithmic_bytes(4) < 0.6 * bf.algorithmic_bytes(4)
    for e in (lane, mx, bf):
        e.close()
