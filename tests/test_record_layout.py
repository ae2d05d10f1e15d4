"""Generation record (include/dropdec.h "Generation record"): the layout the library describes, the dtype Python builds from it, and the
generate() surface that hands it out.  No compute calls (no GPU here)."""
import ctypes as C
import inspect

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from dropoutdecoding_amd import build, _lib
    build.build()
    return _lib.load()


def _fields(lib):
    out, i = [], 0
    while True:
        name, off, cnt, fl = C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
        if lib.dd_record_field(i, C.byref(name), C.byref(off), C.byref(cnt), C.byref(fl)) != 0:
            return out
        out.append((name.value.decode(), off.value, cnt.value, fl.value))
        i += 1


def test_library_exports_the_record_entry_points(lib):
    for s in ("dd_lm_set_record", "dd_record_bytes", "dd_record_field"):
        assert hasattr(lib, s), f"libdropdec.so does not export {s}"


def test_layout_is_four_byte_fields_without_overlap(lib):
    fields = _fields(lib)
    names = [f[0] for f in fields]
    assert names == ["token", "winner", "votes", "K", "base_token", "member_token", "n_drop", "max", "lse", "logprob", "entropy",
                     "base_logprob", "top_id", "top_logit"]
    total = int(lib.dd_record_bytes())
    used = np.zeros(total, dtype=np.int32)
    for name, off, cnt, fl in fields:
        assert off % 4 == 0 and cnt >= 1 and fl in (0, 1), name
        assert off + 4 * cnt <= total, name
        used[off:off + 4 * cnt] += 1
    assert used.max() == 1, "fields overlap"
    by = {f[0]: f for f in fields}
    assert by["member_token"][2] == 64 and by["n_drop"][2] == 64 and by["top_id"][2] == 8 and by["top_logit"][2] == 8
    assert [by[n][3] for n in ("max", "lse", "logprob", "entropy", "base_logprob", "top_logit")] == [1] * 6
    assert [by[n][3] for n in ("token", "winner", "votes", "K", "base_token", "member_token", "n_drop", "top_id")] == [0] * 8
    # past the last field: an error, and the message says which
    assert lib.dd_record_field(len(fields), None, None, None, None) == -1
    assert b"dd_record_field" in lib.dd_last_error()


def test_python_dtype_comes_from_the_library(lib):
    from dropoutdecoding_amd import _lib
    dt = _lib.record_dtype()
    assert dt.itemsize == int(lib.dd_record_bytes())
    for name, off, cnt, fl in _fields(lib):
        f, o = dt.fields[name][0], dt.fields[name][1]
        assert o == off and f.base == (np.float32 if fl else np.int32) and (f.shape == ((cnt,) if cnt > 1 else ()))


def test_generate_surface_carries_the_three_keywords():
    from dropoutdecoding_amd import vlm
    for fn in (vlm.DropoutVLM.generate, vlm.generate_group, vlm.GroupPipeline.run):
        p = inspect.signature(fn).parameters
        for kw in ("return_dict_in_generate", "output_scores", "output_logits"):
            assert kw in p and p[kw].default is False, (fn.__qualname__, kw)
    from dropoutdecoding_amd.lm import DropoutEngine
    for m in ("attach_record", "detach_record", "record"):
        assert callable(getattr(DropoutEngine, m))


def test_result_object_reads_like_a_model_output():
    from dropoutdecoding_amd.vlm import DropoutGenerateOutput
    out = DropoutGenerateOutput(sequences=[[1, 2, 3]], scores=None, logits=("row",), dropout_record={"votes": [3]})
    assert out.sequences == [[1, 2, 3]] and out["sequences"] == [[1, 2, 3]]
    assert out.scores is None and out["logits"] == ("row",) and out.dropout_record["votes"] == [3]
    assert out[0] == [[1, 2, 3]] and out.to_tuple() == ([[1, 2, 3]], ("row",), {"votes": [3]})      # None fields are skipped, as in HF
    assert list(out.keys()) == ["sequences", "scores", "logits", "dropout_record"]
    with pytest.raises(AttributeError):
        out.attentions
