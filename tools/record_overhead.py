"""What an attached generation record (dd_lm_set_record, csrc/dd_record.hip) costs per step: the 64-lane group step and the single-stream
two-sweep step (LLaVA-1.5-7B shapes, K = 8, fp16 cache, synthetic weights), each timed with and without a record in interleaved rounds of
one process (wall time over a run of queued steps, device drained at both ends).  Writes profiles/record_overhead.json.

    python tools/record_overhead.py [steps per round] [rounds] [lanes]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dropoutdecoding_amd import lm
from dropoutdecoding_amd.config import VOTING_NUMBERS_K8

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
LANES = int(sys.argv[3]) if len(sys.argv) > 3 else 64
CAP = 8 + 2 * ROUNDS * (STEPS + 4)
torch.cuda.set_device(0)
engs = []
for i in range(LANES):
    engs.append(lm.DropoutEngine(lm.LLAVA15_7B, family=lm.FAMILY_LLAVA, max_seq=608 + CAP + 32, max_visual=576, kv_format="fp16", seed=50 + i,
                                 share_weights_with=engs[0] if engs else None))
engs[0].load_synthetic(0, 0.02)
embs = [torch.randn(608, 4096, generator=torch.Generator().manual_seed(i)).cuda() for i in range(LANES)]


def timed(step, sync, n):
    for _ in range(3):                     # the eager first step and the graph capture stay outside the timed run
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    sync()
    return (time.perf_counter() - t0) / n * 1e3


def group_round(record):
    for e, x in zip(engs, embs):
        if record:
            e.attach_record(STEPS + 8, scores=True)
        else:
            e.detach_record()
        e.prefill(x, 5, 576)
    g = lm.EngineGroup(engs)
    return timed(lambda: g.decode_step(VOTING_NUMBERS_K8), torch.cuda.synchronize, STEPS)


def solo_round(record):
    e = engs[0]
    e.set_speculation("never")             # the two-sweep step: the un-masked sweep, then the members
    if record:
        e.attach_record(STEPS + 8, scores=True)
    else:
        e.detach_record()
    e.prefill(embs[0], 5, 576)
    ms = timed(lambda: e.decode_step(VOTING_NUMBERS_K8), torch.cuda.synchronize, STEPS)
    e.set_speculation("default")
    return ms


res = {}
for name, fn in ((f"group_step_{LANES}_lanes", group_round), ("single_stream_two_sweep_step", solo_round)):
    t = {False: [], True: []}
    for r in range(ROUNDS):
        for record in (False, True):
            t[record].append(fn(record))
    off, on = statistics.median(t[False]), statistics.median(t[True])
    res[name] = {"ms_without_record": round(off, 4), "ms_with_record": round(on, 4), "ratio": round(on / off, 5),
                 "rounds_without": [round(x, 4) for x in t[False]], "rounds_with": [round(x, 4) for x in t[True]]}
    print(name, json.dumps(res[name]))
for e in engs:
    e.detach_record()
res["setup"] = {"shapes": "LLaVA-1.5-7B, synthetic weights, fp16 cache, K = 8, T0 = 608, scores plane attached", "steps_per_round": STEPS,
                "rounds": ROUNDS, "device": torch.cuda.get_device_name(0)}
out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "record_overhead.json")
if os.environ.get("DD_RECORD_OVERHEAD_OUT"):
    out = os.environ["DD_RECORD_OVERHEAD_OUT"]
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("written:", out)
for e in reversed(engs):
    e.close()
