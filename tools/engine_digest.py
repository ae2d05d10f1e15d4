"""One sha256 per leg over everything a tiny engine computes: the prefill's image logits, every step's base and winning-member
logits, member argmaxes and masks, the emitted tokens and the KV checksums (dd_lm_get).  Two builds of the library compute the
same thing exactly when every line of this script's output is equal: run it on both, on the same machine, and diff.

    python tools/engine_digest.py [formats=bf16,fp8,fp16,mxfp4]

Legs per weight format: solo steps with one (K = 3) and two (K = 12) member sweeps, speculation forced on and off, graph replay
off, fp16 KV cache, group steps with 2 / 3 / 9 / 16 lanes, dd_lm_prefill_group (2 lanes: the per-sequence path; 9 lanes: the batched
GEMMs), truncate + prefill_extend with 5 / 20 / 40 rows, two linked tensor-parallel ranks (16-bit formats), and seeded random
matrices through the format's loader instead of the synthetic fill.  Any error ends the run.
"""
from __future__ import annotations

import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from dropoutdecoding_amd import _lib
from dropoutdecoding_amd.lm import DropoutEngine, EngineGroup, LMConfig, TensorParallelGroup, prefill_group

CFG = LMConfig(vocab_size=1000, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4, num_kv_heads=2)
MAX_SEQ, MAX_VISUAL, T0, SPAN, STEPS = 256, 32, 40, (8, 24), 6
K3 = [0.1, 0.3, 0.5]
K12 = [0.05 * (i + 1) for i in range(12)]


def rows(n: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, CFG.hidden_size, generator=g).cuda()


def state_dict(seed: int = 11) -> dict:
    g = torch.Generator().manual_seed(seed)
    d, ff, q, kv = CFG.hidden_size, CFG.intermediate_size, CFG.num_heads * 128, CFG.num_kv_heads * 128
    rnd = lambda r, c: (torch.randn(r, c, generator=g) * 0.05).to(torch.bfloat16)
    sd = {"model.embed_tokens.weight": rnd(CFG.vocab_size, d), "model.norm.weight": 1 + rnd(1, d)[0], "lm_head.weight": rnd(CFG.vocab_size, d)}
    for i in range(CFG.num_layers):
        p = f"model.layers.{i}."
        sd.update({p + "input_layernorm.weight": 1 + rnd(1, d)[0], p + "post_attention_layernorm.weight": 1 + rnd(1, d)[0],
                   p + "self_attn.q_proj.weight": rnd(q, d), p + "self_attn.k_proj.weight": rnd(kv, d),
                   p + "self_attn.v_proj.weight": rnd(kv, d), p + "self_attn.o_proj.weight": rnd(d, q),
                   p + "mlp.gate_proj.weight": rnd(ff, d), p + "mlp.up_proj.weight": rnd(ff, d), p + "mlp.down_proj.weight": rnd(d, ff)})
    return sd


class Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, *arrays) -> None:
        for a in arrays:
            self.h.update(np.ascontiguousarray(a).tobytes())

    def prefilled(self, e: DropoutEngine) -> None:
        self.add(e.image_logits(), e.logits(), e.hidden(), e.tokens(), e.kv_sums())

    def stepped(self, e: DropoutEngine) -> None:
        self.add(e.base_logits(), e.logits(), e.tokens(), e.kv_sums())
        if e._last_K:
            s = e.last_step()
            self.add(s["drop"], s["keep"], s["member_argmax"], [s["winner"], s["voted"]])


def engine(fmt: str, seed: int = 1, **kw) -> DropoutEngine:
    return DropoutEngine(CFG, max_seq=MAX_SEQ, max_visual=MAX_VISUAL, seed=seed, weight_format=fmt, **kw)


def solo(fmt, mprobs, spec="default", graph=1, kv="fp32", real=False):
    lib = _lib.load()
    lib.dd_set_tuning(8, graph)
    try:
        e = engine(fmt, kv_format=kv)
        e.load_state_dict(state_dict()) if real else e.load_synthetic(3, 0.05)
        e.set_speculation(spec)
        dg = Digest()
        e.prefill(rows(T0, 7), *SPAN)
        dg.prefilled(e)
        for _ in range(STEPS):
            e.decode_step(mprobs)
            dg.stepped(e)
        e.close()
        return dg
    finally:
        lib.dd_set_tuning(8, 1)


def lanes_of(fmt, n):
    owner = engine(fmt)
    owner.load_synthetic(3, 0.05)
    return [owner] + [engine(fmt, seed=1 + i, share_weights_with=owner) for i in range(1, n)]


def group(fmt, n, mprobs, batched_prefill=False):
    E = lanes_of(fmt, n)
    dg = Digest()
    xs = [rows(T0 - (i % 3), 20 + i) for i in range(n)]
    if batched_prefill:
        prefill_group(E, xs, [SPAN] * n)
    else:
        for e, x in zip(E, xs):
            e.prefill(x, *SPAN)
    for e in E:
        dg.prefilled(e)
    grp = EngineGroup(E)
    for _ in range(STEPS):
        grp.decode_step(mprobs)
        for e in E:
            dg.stepped(e)
    for e in reversed(E):
        e.close()
    return dg


def extend(fmt):
    e = engine(fmt)
    e.load_synthetic(3, 0.05)
    dg = Digest()
    e.prefill(rows(T0, 7), *SPAN)
    for n in (5, 20, 40):                       # the decode GEMVs twice (8- and 32-row form), the GEMM path once
        e.truncate(SPAN[0] + SPAN[1])
        e.prefill_extend(rows(n, 30 + n))
        dg.add(e.logits(), e.hidden(), e.tokens(), e.kv_sums())
        e.decode_step(K3)
        dg.stepped(e)
    e.close()
    return dg


def tp(fmt):
    g = TensorParallelGroup(CFG, 2, max_seq=MAX_SEQ, max_visual=MAX_VISUAL, seed=1, weight_format=fmt)
    g.load_state_dict(state_dict())
    dg = Digest()
    g.prefill(rows(T0, 7), *SPAN)
    for e in g.ranks:
        dg.prefilled(e)
    for _ in range(STEPS):
        g.decode_step(K3)
        for e in g.ranks:
            dg.stepped(e)
    g.close()
    return dg


LEGS = [
    ("solo_K3", lambda f: solo(f, K3)),
    ("solo_K12", lambda f: solo(f, K12)),
    ("solo_K0", lambda f: solo(f, [])),
    ("spec_always", lambda f: solo(f, K3, spec="always")),
    ("spec_never", lambda f: solo(f, K3, spec="never")),
    ("no_graph_always", lambda f: solo(f, K3, spec="always", graph=0)),
    ("no_graph_never", lambda f: solo(f, K3, spec="never", graph=0)),
    ("kv_fp16", lambda f: solo(f, K3, kv="fp16")),
    ("group_2", lambda f: group(f, 2, K3)),
    ("group_3_K3", lambda f: group(f, 3, K3)),
    ("group_9", lambda f: group(f, 9, K12[:8])),
    ("group_16_K3", lambda f: group(f, 16, K3)),
    ("prefill_group_2", lambda f: group(f, 2, K3, batched_prefill=True)),
    ("prefill_group_9", lambda f: group(f, 9, K3, batched_prefill=True)),
    ("extend_5_20_40", extend),
    ("tp_2_ranks", tp),
    ("loader_real_weights", lambda f: solo(f, K3, real=True)),
]


def main() -> int:
    formats = ["bf16", "fp8", "fp16", "mxfp4"]
    for a in sys.argv[1:]:
        if a.startswith("formats="):
            formats = a.split("=", 1)[1].split(",")
    for fmt in formats:
        for name, leg in LEGS:
            if name == "tp_2_ranks" and fmt in ("fp8", "mxfp4"):       # shards keep 16-bit matrices
                continue
            out = leg(fmt).h.hexdigest()
            print(f"{fmt:6s} {name:20s} {out}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
