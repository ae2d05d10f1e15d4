"""MXFP4 weight storage, host side: the quantiser (lm.quantize_mxfp4 / dequantize_mxfp4) and the C-ABI entry point.  No GPU."""
import ctypes

import torch

from dropoutdecoding_amd.lm import dequantize_mxfp4, quantize_mxfp4


def test_round_trip_is_idempotent_and_bf16_exact():
    g = torch.Generator().manual_seed(2)
    w = torch.randn(48, 256, generator=g) * 0.05
    w[5] *= 1e-3                                            # rows of another magnitude: other block exponents
    w[6] *= 300.0
    q, s = quantize_mxfp4(w)
    assert q.dtype == torch.uint8 and q.shape == (48, 128) and s.dtype == torch.uint8 and s.shape == (48, 8)
    assert int(s.min()) >= 7 and int(s.max()) <= 247
    d = dequantize_mxfp4(q, s)
    assert d.dtype == torch.float32 and d.shape == w.shape
    assert torch.equal(d, d.bfloat16().float())             # e2m1 x a power of two: exact in bf16
    q2, s2 = quantize_mxfp4(d)
    assert torch.equal(q2, q) and torch.equal(s2, s)
    assert torch.equal(dequantize_mxfp4(q2, s2), d)
    # the block maximum lands in the top binade of e2m1, so no element is off by more than half a step of that binade
    blk = (w - d).reshape(48, 8, 32).abs().amax(2) / w.reshape(48, 8, 32).abs().amax(2)
    assert float(blk.max()) <= 0.25


def test_rounding_ties_go_to_the_even_code_and_large_values_saturate():
    """e = floor(log2(7)) - 2 = 0: the elements are rounded as they stand.  The midpoints between two e2m1 values go to the value
    with the even code: 0.25 -> 0 (code 0), 0.75 -> 1 (code 2), 1.25 -> 1, 1.75 -> 2 (code 4), 2.5 -> 2, 3.5 -> 4 (code 6), 5 -> 4.
    (0.26 and 0.74 are NOT ties: 0.5 is an e2m1 value and the nearest one to both.)"""
    vals = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, 7.0, -7.0, 0.26, 0.74, -0.25, -0.75, -5.0, 0.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0, 6.0, -6.0, 0.5, 0.5, -0.0, -1.0, -4.0, 0.0]
    b = torch.zeros(1, 32)
    b[0, :len(vals)] = torch.tensor(vals)
    q, s = quantize_mxfp4(b)
    assert s.tolist() == [[127]]
    got = dequantize_mxfp4(q, s)[0]
    assert got[:len(vals)].tolist() == want
    assert torch.signbit(got[12]) and float(got[16:].abs().max()) == 0.0       # the sign is kept, the rest of the block is zero
    # packing: element 2j in the low nibble of byte j; 0.25 -> code 0, 0.75 -> code 2, 1.25 -> code 2, 1.75 -> code 4
    assert q[0, :2].tolist() == [0 | (2 << 4), 2 | (4 << 4)]
    assert q[0, 4].item() == (7 | (15 << 4))                # 7.0 -> +6 (code 7), -7.0 -> -6 (code 15)


def test_zero_blocks_and_exponent_clamps():
    w = torch.zeros(2, 64)
    w[1, 32:] = torch.linspace(-1, 1, 32) * 2.0 ** 126     # beyond exponent 120: clamped scale, elements saturate
    w[1, 0] = 2.0 ** -140                                   # below exponent -120
    q, s = quantize_mxfp4(w)
    assert s.tolist() == [[7, 7], [7, 247]]
    d = dequantize_mxfp4(q, s)
    assert float(d[0].abs().max()) == 0.0 and float(d[1, :32].abs().max()) == 0.0
    assert float(d[1, 32:].abs().max()) == 6.0 * 2.0 ** 120
    for bad in (torch.zeros(4, 48), torch.zeros(64)):
        try:
            quantize_mxfp4(bad)
        except ValueError:
            continue
        raise AssertionError("K must be a multiple of 32 and the input a matrix")


def test_entry_point_is_bound_and_exported_by_both_libraries():
    from dropoutdecoding_amd import _lib, build
    build.build()
    assert "dd_lm_load_tensor_mxfp4" in _lib.SYMBOLS
    for path in (_lib.LIB_PATH, _lib.TOOLS_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), "dd_lm_load_tensor_mxfp4"), path       # plain dlopen: no compute calls without a GPU
    assert len(_lib.load().dd_lm_load_tensor_mxfp4.argtypes) == 8
