"""Decode GEMVs of the engine in isolation (dd_lm_time_gemv: HIP events, weights cycled over the 32 layers):
per matrix and row count, the whole GEMV (streaming kernel + finishing kernel) and the streaming kernel alone.
formats=bf16,fp8,mxfp4 [repeats=R] [json=path]: one engine per weight format at LLaVA-1.5-7B shapes (K = 4096 / 11008), the formats
timed alternately R times in one process; median, min and max per (format, rows, matrix), TB/s from the format's bytes per parameter."""
import json, os, statistics, sys
os.environ.setdefault("DD_USE_TOOLS_LIB", "1")      # timing hooks / experiment knobs: libdropdec_tools.so
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dropoutdecoding_amd import lm

torch.cuda.set_device(0)
from dropoutdecoding_amd import _lib
row_sets = (8, 16, 32, 64, 72)
formats, repeats, json_path = None, 5, None
for kv in sys.argv[1:]:                      # key=value: dd_tools_set_tuning; rows=64: only that pass width
    k_, v_ = kv.split("=")
    if k_ == "rows":
        row_sets = tuple(int(r) for r in v_.split(","))
    elif k_ == "formats":
        formats = v_.split(",")
    elif k_ == "repeats":
        repeats = int(v_)
    elif k_ == "json":
        json_path = v_
    else:
        _lib.load().dd_tools_set_tuning(int(k_), int(v_))
names = {0: "qkv", 1: "o_proj", 2: "gate/up", 3: "down"}
C5 = os.environ.get("DD_AB_MODEL", "") == "mistral-fp8"       # BASELINE config 5's matrices: Mistral-7B shapes, fp8 tiles


def engine(fmt):
    e = lm.DropoutEngine(lm.MISTRAL_7B if C5 else lm.LLAVA15_7B, family=lm.FAMILY_NEXT if C5 else lm.FAMILY_LLAVA, max_seq=784, max_visual=576,
                         kv_format="fp16", weight_format=fmt)
    e.load_synthetic(0, 0.02)
    e.prefill(torch.randn(608, 4096, generator=torch.Generator().manual_seed(0)).cuda(), 5, 576)
    return e


if formats is None:
    e = engine("fp8" if C5 else "bf16")
    for rows in row_sets:
        out = []
        for which in range(4):
            ms, by = e.time_gemv(which, rows, 96)
            ms_s = e.time_gemv(which + 8, rows, 96)[0] if rows >= 16 else ms
            out.append(f"{names[which]} {ms * 1e3:6.1f} us ({by / ms / 1e9 * 1e3 / 1e3:5.2f} TB/s; streaming kernel {ms_s * 1e3:5.1f} us = {by / ms_s / 1e9:5.2f} TB/s)")
        print(f"{rows:2d} rows: " + " | ".join(out), flush=True)
    sys.exit(0)

if row_sets == (8, 16, 32, 64, 72):
    row_sets = (8, 16)                       # the widths every format has a kernel for
engines = {f: engine(f) for f in formats}
for f in formats:                            # warm-up: every kernel of every format once, not recorded
    for rows in row_sets:
        for which in range(4):
            engines[f].time_gemv(which, rows, 32)
us, nbytes = {}, {}
for r in range(repeats):
    for f in formats:                        # alternating: drift of the device lands on every format alike
        for rows in row_sets:
            for which in range(4):
                ms, by = engines[f].time_gemv(which, rows, 96)
                us.setdefault((f, rows, which), []).append(ms * 1e3)
                nbytes[(f, which)] = by
res = {"model": "mistral-7b" if C5 else "llava-1.5-7b", "iters_per_sample": 96, "repeats": repeats, "unit": "us per launch (HIP events, mean of 96 launches over the 32 layers)",
       "bytes_per_param": {"bf16": 2.0, "fp16": 2.0, "fp8": 1.0, "mxfp4": 0.5 + 1.0 / 32}, "results": []}
for rows in row_sets:
    for which in range(4):
        line = []
        for f in formats:
            v = us[(f, rows, which)]
            med = statistics.median(v)
            rec = {"format": f, "rows": rows, "matrix": names[which], "median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                   "bytes": nbytes[(f, which)], "tb_per_s": round(nbytes[(f, which)] / med / 1e6, 3)}
            res["results"].append(rec)
            line.append(f"{f} {med:6.1f} us [{min(v):.1f} .. {max(v):.1f}] {rec['tb_per_s']:5.2f} TB/s")
        print(f"{rows:2d} rows {names[which]:8s}: " + " | ".join(line), flush=True)
if json_path:
    os.makedirs(os.path.dirname(os.path.abspath(json_path)), exist_ok=True)
    with open(json_path, "w") as fh:
        json.dump(res, fh, indent=1)
