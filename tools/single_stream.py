"""One image at a time (the reference's loop): decoded tokens/s over several images, and how often the speculative
single-sweep step held.  python tools/single_stream.py [n_images] [spec 0/1]
python tools/single_stream.py [n_images] formats=bf16,fp8,mxfp4 [repeats=R] [json=path]: one model per weight format (LLaVA-1.5-7B shapes,
synthetic weights), two-sweep (spec 0) and speculative (spec 1) tokens/s, the formats timed alternately R times in one process."""
import json, os, statistics, sys, time
os.environ.setdefault("DD_USE_TOOLS_LIB", "1")      # timing hooks / experiment knobs: libdropdec_tools.so
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import synthetic_inputs
from dropoutdecoding_amd import config as ddcfg, _lib
from dropoutdecoding_amd.llava import CustomLlavaForConditionalGeneration

torch.cuda.set_device(0)
pos = [a for a in sys.argv[1:] if "=" not in a]
opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
n_img = int(pos[0]) if len(pos) > 0 else 5
spec = int(pos[1]) if len(pos) > 1 else 1
ddcfg.settings["voting_numbers"] = ddcfg.VOTING_NUMBERS_K8
n_new = 128


def build(fmt=None):
    if fmt is not None:
        ddcfg.settings["weight_format"] = fmt
    try:
        return CustomLlavaForConditionalGeneration.from_synthetic(max_new_tokens=136)
    finally:
        if fmt is not None:
            ddcfg.settings.pop("weight_format", None)


def one(model, i):
    ids, px = synthetic_inputs(i, model.engine.cfg.vocab_size, model.image_token_index)
    return model.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), max_new_tokens=n_new, eos_token_id=[])


def tok_s(model, first):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_img):
        one(model, first + i)
    torch.cuda.synchronize()
    return n_img * n_new / (time.perf_counter() - t0)


if "formats" in opts:
    formats, repeats = opts["formats"].split(","), int(opts.get("repeats", 3))
    models = {f: build(f) for f in formats}
    for sp in (0, 1):
        _lib.load().dd_tools_set_tuning(14, sp)
        for f in formats:
            one(models[f], 0)                # warm-up: graphs captured, not recorded
    rate = {}
    for r in range(repeats):
        for sp in (0, 1):
            _lib.load().dd_tools_set_tuning(14, sp)
            for f in formats:                # alternating formats inside every round
                rate.setdefault((f, sp), []).append(tok_s(models[f], 1 + r * n_img))
    res = {"model": "llava-1.5-7b shapes, synthetic weights, K = 8", "images_per_sample": n_img, "new_tokens": n_new, "repeats": repeats, "results": []}
    for f in formats:
        for sp in (0, 1):
            v = rate[(f, sp)]
            res["results"].append({"format": f, "step": "speculative" if sp else "two-sweep", "median_tok_s": round(statistics.median(v), 1),
                                   "min_tok_s": round(min(v), 1), "max_tok_s": round(max(v), 1)})
            print(f"{f:6s} {'speculative' if sp else 'two-sweep  '}: {statistics.median(v):6.1f} tok/s [{min(v):.1f} .. {max(v):.1f}]", flush=True)
    if "json" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["json"])), exist_ok=True)
        with open(opts["json"], "w") as fh:
            json.dump(res, fh, indent=1)
    sys.exit(0)

model = build()
_lib.load().dd_tools_set_tuning(14, spec)
eng = model.engine
one(model, 0)
print(f"spec={spec}: {n_img} images, {(r := tok_s(model, 1)):.1f} tok/s, {n_new / r * 1e3:.1f} ms per image")
# success rate of the speculation on one more image, step by step
ids, px = synthetic_inputs(99, eng.cfg.vocab_size, model.image_token_index)
model._prepare(ids.cuda(), n_new, None, 1, [], False, dict(pixel_values=px.cuda()))
oks = []
for _ in range(64):
    eng.decode_step()
    oks.append(eng.spec_ok())
print("speculation held in", sum(oks), "of", len(oks), "steps")
