"""One lane of the engine against its own `RefDecoder`, step by step (helper of the oracle-anchored GPU tests; no tests here).

  token ids, keep sets, mask flags, masked counts, member argmax ids, winner   exact
  prefill / image-span / winner's / un-masked logits                          <= TOL = 1e-3 of max |logit| (north star)
  epistemic uncertainties                                                      rtol 5e-3, atol 1e-6

A discrete result may differ from the oracle's only where the ORACLE ITSELF puts the decision AT THE ELEMENT THAT DIFFERS inside the
logits tolerance.  The lane then leaves the comparison from that step on (`live = False`, `excuse` says why); `report()` prints and
warns every excuse and fails when more than one lane in eight has one.  What counts as a near-tie, per kind of result:

  top-k ids of an image row   the row's k-th minus (k+1)-th largest oracle logit < TOL of the row's max |logit| (`topk_note`: not an
                              excuse by itself — only a keep set can feel it)
  keep set                    with a `topk_note`: every differing row must be one of the rows the note names (the flag is "argmax of
                              the un-masked logits is among the row's top-k ids": only those rows have other ids); without one: the
                              un-masked logits' top-1 minus top-2 < TOL of their max |logit| (the argmax itself is the tie)
  mask flags                  at EVERY (member, token) whose flag differs, the uniform is closer to its drop probability than
                              `p_limit` = max(1e-5, twice what the two sides' fp32 uncertainties move the probabilities by) —
                              InstructBLIP (no draws): that token's uncertainty is closer than `p_limit` of the uncertainties' range
                              to that member's quantile threshold.  LLaVA-1.5's masks accumulate over the members (llava.py:654-657),
                              so there the rule applies to the FIRST member whose flag differs at a token; the later members' flags at
                              that token are that same decision carried along
  member argmax ids           for EVERY member whose id differs, top-1 minus top-2 of what that member's argmax ran over
                              (`StepRecord.member_margin[m]`) < TOL

The streams are seeded, so a given tree either has such a near-tie or not: no flake.
"""
import warnings

import numpy as np

from oracle.decode_ref import FAMILY_LLAVA

TOL = 1e-3                            # logits: relative to the largest |logit| (BASELINE north_star)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def top_gap(v):
    v = np.asarray(v, np.float64)
    t = np.partition(v, -2)[-2:]
    return float((t[1] - t[0]) / np.abs(v).max())


def thresholds(epi, probs):
    """drop probabilities of models/llava.py:641-647 in float64: p = 0.1 + (mprob - 0.1) (e - lo) / (hi - lo)"""
    e = np.asarray(epi, np.float64)
    return 0.1 + (np.asarray(probs, np.float64)[:, None] - 0.1) * ((e - e.min()) / np.ptp(e))[None]


def mask_distance(r, ref, probs):
    """[K, L]: how far the oracle's mask decision of (member, token) sits from flipping."""
    if r.uniforms is None:            # InstructBLIP: drop where e >= quantile(e, 1 - p) (instructblip.py:450-453): how close an uncertainty sits to a threshold
        e = ref.epi.numpy().astype(np.float64)
        thr = np.quantile(e, 1.0 - np.asarray(probs, np.float64))
        d = np.abs(e[None, :] - thr[:, None])
        d[d == 0.0] = np.inf          # (a threshold that IS an element — weight 0 of the interpolation — is the same element on both sides)
        return d / np.ptp(e)
    return np.abs(r.uniforms.astype(np.float64) - thresholds(ref.epi.numpy(), probs))


class LaneCheck:
    """One lane's step-by-step comparison with its oracle; `live` turns False at an excused near-tie."""

    def __init__(self, name, eng, ref, probs):
        self.name, self.eng, self.ref, self.probs = name, eng, ref, probs
        self.live, self.excuse, self.worst = True, None, 0.0
        self.topk_note, self.topk_rows = None, []   # the image span's top-k id sets differ at a near-tie: only the keep sets can feel it
        self.p_limit = 1e-5             # a uniform this close to its threshold may flip (set from the two sides' uncertainties in prefill())
        self.prefill_err = (0.0, 0.0)   # (last-row logits, image-span logits)

    def _excused(self, what, margin, limit, s):
        """A discrete result differs: a wrong result unless the oracle's margin AT THAT ELEMENT is under the limit."""
        info = f"{self.name} step {s}: {what} from the oracle; the oracle's margin at that decision is {margin:.3g}"
        assert margin < limit, info + f" (>= {limit:g}: not a near-tie — wrong result)"
        self.live, self.excuse = False, info

    def prefill(self):
        e, r = self.eng, self.ref
        err = relerr(e.logits(), r.prefill_logits[-1].numpy())
        assert err <= TOL, f"{self.name}: prefill logits {err:.3g}"
        err_img = relerr(e.image_logits(), r.image_logits.numpy())
        assert err_img <= TOL, f"{self.name}: image-span logits {err_img:.3g}"
        self.prefill_err = (err, err_img)
        np.testing.assert_allclose(e.vision_uncert_dict()["epis_uncert_per_token"][0], r.epi.numpy(), rtol=5e-3, atol=1e-6,
                                   err_msg=f"{self.name}: epistemic uncertainty")
        img = np.sort(r.image_logits.numpy(), axis=1)[:, ::-1]
        k = r.topk_ids.shape[1]
        # the thresholds divide by (max - min) of the uncertainties — a few per cent of their size for these weights — so the last bits
        # of the two sides' fp32 uncertainties move a threshold by up to p_err: a uniform closer than that to its threshold is a tie
        p_err = float(np.abs(thresholds(e.vision_uncert_dict()["epis_uncert_per_token"][0], self.probs) - thresholds(r.epi.numpy(), self.probs)).max())
        assert p_err < 2e-4, f"{self.name}: thresholds from the two sides' uncertainties differ by {p_err:.3g}"
        self.p_limit = max(1e-5, 2 * p_err)
        got, want = np.sort(e.topk()[1], 1), np.sort(r.topk_ids.numpy(), 1)
        if not np.array_equal(got, want):
            rows = np.nonzero((got != want).any(axis=1))[0]                                  # the top-k boundary (llava.py:310)
            rgap = ((img[rows, k - 1] - img[rows, k]) / np.abs(img[rows]).max(axis=1)).max()
            assert rgap < TOL, f"{self.name}: top-k ids of image rows {rows.tolist()} differ from the oracle, boundary gap {rgap:.3g}"
            self.topk_rows = rows.tolist()
            self.topk_note = f"top-k ids of image rows {self.topk_rows} differ at a boundary gap of {rgap:.3g}"

    def _keep(self, st, r, s):
        if np.array_equal(st["keep"], r.keep):
            return True
        rows = np.nonzero(np.asarray(st["keep"]) != np.asarray(r.keep))[0].tolist()
        what = f"keep set (argmax of the un-masked logits in the rows' top-k ids) differs at image rows {rows}"
        if self.topk_note:
            assert set(rows) <= set(self.topk_rows), (f"{self.name} step {s}: {what}, not all of them rows whose top-k ids differ "
                                                      f"({self.topk_note}) — wrong result")
            self.live, self.excuse = False, f"{self.name} step {s}: {what} from the oracle ({self.topk_note})"
        else:
            self._excused(what, top_gap(r.base_logits), TOL, s)
        return False

    def _masks(self, st, r, s):
        diff = np.asarray(st["drop"]) != np.asarray(r.drop)
        if not diff.any():
            return True
        if self.ref.family == FAMILY_LLAVA:                  # masks accumulate over the members (oracle/dropout_ref.py sample_masks:
            diff &= np.cumsum(diff, axis=0) == 1             # `running` is not reset): the first member whose flag differs at a token decides
        where = np.argwhere(diff)
        margin = float(mask_distance(r, self.ref, self.probs)[diff].max())   # the WORST of the differing elements must be a near-tie
        self._excused(f"mask flags differ at (member, token) {where.tolist()}", margin, self.p_limit, s)
        return False

    def _members(self, st, r, s):
        got, want = np.asarray(st["member_argmax"]), np.asarray(r.member_argmax)
        if np.array_equal(got, want):
            return True
        ms = np.nonzero(got != want)[0].tolist()
        margin = max(r.member_margin[m] for m in ms) if r.member_margin else 1.0
        self._excused(f"member argmax ids differ at members {ms}", margin, TOL, s)
        return False

    def step(self, s):
        if not self.live:
            return
        e, r = self.eng, self.ref.records[s]
        st = e.last_step()
        err = relerr(e.base_logits(), r.base_logits)
        assert err <= TOL, f"{self.name} step {s}: un-masked logits {err:.3g}"
        self.worst = max(self.worst, err)
        if not self._keep(st, r, s) or not self._masks(st, r, s):
            return
        assert st["masked_numbers"].tolist() == r.masked_numbers, f"{self.name} step {s}: masked counts"
        if not self._members(st, r, s):
            return
        assert st["winner"] == r.winner, f"{self.name} step {s}: winner"
        err = relerr(e.logits(), r.logits)
        assert err <= TOL, f"{self.name} step {s}: winner's logits {err:.3g}"
        self.worst = max(self.worst, err)

    def tokens(self):
        if self.live:
            assert self.eng.tokens() == self.ref.tokens_out, f"{self.name}: token ids"


def report(checks, what, max_gone=None):
    """Print the summary, emit it as a UserWarning too (a `pytest -q` log summarises warnings at the end of the run), and fail when more
    than one lane in eight (or `max_gone`: a test of ONE lane has no eighth) left the comparison at a near-tie."""
    gone = [c for c in checks if not c.live]
    lines = [f"{what}: {len(checks) - len(gone)} of {len(checks)} lanes compared to the end, worst logits error: prefill "
             f"{max(c.prefill_err[0] for c in checks):.2e}, image span {max(c.prefill_err[1] for c in checks):.2e}, steps "
             f"{max(c.worst for c in checks):.2e} (tolerance {TOL:g})"]
    lines += [f"  excused: {c.excuse}" for c in gone]
    lines += [f"  note: {c.name}: {c.topk_note}; no keep set felt it" for c in checks if c.topk_note and c.live]
    print("\n" + "\n".join(lines))
    warnings.warn(UserWarning("\n".join(lines)))
    assert len(gone) <= (len(checks) // 8 if max_gone is None else max_gone), f"{what}: {len(gone)} lanes left the comparison at near-ties"
