"""tests/lane_check.py on made-up lanes (no GPU): a discrete difference is excused only by a near-tie AT THE ELEMENT THAT DIFFERS — a
near-tie somewhere else in the step, at another member or at another image row must not excuse it."""
import numpy as np
import pytest
import torch

from oracle.decode_ref import FAMILY_LLAVA, FAMILY_NEXT, StepRecord

from lane_check import LaneCheck, report          # tests/lane_check.py

K, L, V = 3, 6, 16
PROBS = [0.3, 0.5, 0.7]


class _Ref:
    def __init__(self, family, rec):
        self.family, self.records, self.tokens_out = family, [rec], [0, int(rec.token)]
        self.epi = torch.linspace(1.0, 2.0, L)


class _Eng:
    def __init__(self, rec):
        self.st = {"drop": rec.drop.copy(), "keep": rec.keep.copy(), "masked_numbers": np.asarray(rec.masked_numbers),
                   "member_argmax": np.asarray(rec.member_argmax), "winner": rec.winner}
        self.base, self.win = rec.base_logits.copy(), rec.logits.copy()

    def last_step(self):
        return self.st

    def base_logits(self):
        return self.base

    def logits(self):
        return self.win


def _lane(family=FAMILY_NEXT):
    from lane_check import thresholds
    rs = np.random.RandomState(1)
    logits = rs.standard_normal(V).astype(np.float32)
    logits[3] = 4.0                                                   # a clear argmax
    p = thresholds(np.linspace(1.0, 2.0, L), PROBS)
    uni = (p + 0.2).astype(np.float32)                                # far from every threshold: nothing dropped
    uni[1, 2] = np.float32(p[1, 2] + 2e-6)                            # ONE near-tie: member 1, token 2
    rec = StepRecord(3, np.zeros(L, bool), uni, np.zeros((K, L), bool), [0] * K, [3] * K, 0, 3, logits.copy(), logits.copy(), {},
                     [0.5, 1e-5, 0.5])                                # member 1's argmax is a near-tie, the others are not
    ref = _Ref(family, rec)
    eng = _Eng(rec)
    return LaneCheck("made-up lane", eng, ref, PROBS), eng


def test_equal_lane_stays_live():
    c, _ = _lane()
    c.step(0)
    assert c.live and c.excuse is None


@pytest.mark.parametrize("family", [FAMILY_NEXT, FAMILY_LLAVA])
def test_mask_flag_is_excused_only_at_its_own_near_tie(family):
    c, eng = _lane(family)
    eng.st["drop"][1, 2] = True                                       # the near-tie itself
    c.step(0)
    assert not c.live and "(member, token) [[1, 2]]" in c.excuse
    c, eng = _lane(family)
    eng.st["drop"][0, 4] = True                                       # another element, with the near-tie elsewhere in the same step
    with pytest.raises(AssertionError, match="not a near-tie"):
        c.step(0)
    c, eng = _lane(family)
    eng.st["drop"][1, 2] = eng.st["drop"][2, 5] = True                # the near-tie and a wrong flag together
    with pytest.raises(AssertionError, match="not a near-tie"):
        c.step(0)


def test_cumulative_masks_carry_the_first_members_decision():
    c, eng = _lane(FAMILY_LLAVA)
    eng.st["drop"][1:, 2] = True                                      # LLaVA-1.5: member 2 inherits member 1's flag at token 2
    c.step(0)
    assert not c.live
    c, eng = _lane(FAMILY_NEXT)                                       # masks reset per member: member 2's flag is its own decision
    eng.st["drop"][1:, 2] = True
    with pytest.raises(AssertionError, match="not a near-tie"):
        c.step(0)


def test_member_argmax_is_excused_only_by_that_members_margin():
    c, eng = _lane()
    eng.st["member_argmax"][1] = 7
    c.step(0)
    assert not c.live and "members [1]" in c.excuse
    c, eng = _lane()
    eng.st["member_argmax"][2] = 7                                    # member 2's margin is 0.5; member 1's near-tie must not excuse it
    with pytest.raises(AssertionError, match="not a near-tie"):
        c.step(0)


def test_keep_set_with_a_topk_note_is_excused_only_at_the_noted_rows():
    c, eng = _lane()
    c.topk_note, c.topk_rows = "top-k ids of image rows [4] differ at a boundary gap of 1e-05", [4]
    eng.st["keep"][4] = True
    c.step(0)
    assert not c.live and "rows [4]" in c.excuse
    c, eng = _lane()
    c.topk_note, c.topk_rows = "top-k ids of image rows [4] differ at a boundary gap of 1e-05", [4]
    eng.st["keep"][1] = True                                          # (before: a note excused EVERY later keep-set difference)
    with pytest.raises(AssertionError, match="wrong result"):
        c.step(0)
    c, eng = _lane()
    eng.st["keep"][1] = True                                          # no note, a clear argmax
    with pytest.raises(AssertionError, match="not a near-tie"):
        c.step(0)


def test_report_warns_and_caps_the_excused_lanes():
    lanes = [_lane() for _ in range(8)]
    lanes[0][1].st["member_argmax"][1] = 7
    for c, _ in lanes:
        c.step(0)
    with pytest.warns(UserWarning, match="7 of 8 lanes compared to the end"):
        report([c for c, _ in lanes], "made-up group")
    lanes[1][0].live = False
    with pytest.warns(UserWarning), pytest.raises(AssertionError, match="2 lanes left"):
        report([c for c, _ in lanes], "made-up group")
