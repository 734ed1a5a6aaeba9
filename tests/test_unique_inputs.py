"""The staircase cases of tests/test_gpu_unique.py can tell a wrong winner kernel from a right one -- shown on the
reference alone, without a device.

The winner kernel keeps, per lane, its best entry and its runner-up's value, and leaves jb - 1, jb, jb + 1 out of the
rival minimum.  Two wrong kernels are restated in unique_ref (rivals="all": nothing left out; rivals="lanes": the
whole lane of an excluded entry left out, i.e. no fall-back to the runner-up).  WITNESSES pins, for one (penalties,
ratio) per case, how many verdicts the first changes and how many m2 the second changes.  Not every combination of
case, penalties and ratio the device file runs shows every effect (a P2 no path ever pays leaves the aggregated curve
without a second minimum 64 disparities away; at ratio 60 and P = 0 nearly every node fails under either rival set), so
for each case and ratio the conditions are asked of its penalty variants together."""
import numpy as np
import pytest

from unique_inputs import RATIOS, STAIRCASES, VARIANTS, case, reference

# (case, variant, ratio): (failing, passing contested nodes, verdicts changed by "all", m2 changed by "lanes")
WITNESSES = {
    ("129-left", "none", 15): (69, 247, 119, 9),
    ("129-left", "sgm", 15): (8, 308, 134, 5),
    ("256-right", "none", 15): (198, 1002, 104, 9),
    ("257-left", "sgm", 60): (186, 1620, 248, 59),
    ("seams-left", "none", 15): (6298, 18832, 10128, 463),
    ("seams-left", "sgm", 15): (642, 24488, 8405, 138),
    ("2048-left", "none", 15): (1028, 1262, 655, 66),
}


def figures(name, variant, ratio):
    r = reference(name, variant, ratio)
    node = case(name)[5][2]
    ra, rl = reference(name, variant, ratio, rivals="all"), reference(name, variant, ratio, rivals="lanes")
    passing = r["contested"] & ~r["fail"]
    return (int(r["fail"].sum()), int(passing.sum()), int((ra["fail"] != r["fail"]).sum()),
            int(((rl["m2"] != r["m2"]) & node).sum()))


@pytest.mark.parametrize("key", sorted(WITNESSES))
def test_witness_rows(key):
    name, variant, ratio = key
    got = figures(name, variant, ratio)
    assert got == WITNESSES[key]
    assert got[0] >= 5 and got[1] >= 5 and got[2] >= 1
    assert case(name)[4] > 64 and got[3] >= 1
    r, rl = reference(name, variant, ratio), reference(name, variant, ratio, rivals="lanes")
    assert (r["conf"] != rl["conf"]).any()   # ... hence the confidence


@pytest.mark.parametrize("name", [n for n in STAIRCASES if n != "600-left-levels"])
def test_every_case_and_ratio_the_device_file_runs(name):
    assert set(RATIOS) == {0, 15, 60, 100}
    nd = case(name)[4]
    for ratio in (r for r in RATIOS if 0 < r < 100):
        f = np.array([figures(name, v, ratio) for v in ("sgm", "none")])   # ("zero" has the verdicts of "none")
        assert (f[:, 0] >= 5).any() and (f[:, 1] >= 5).any(), (name, ratio, f.tolist())
        assert (f[:, 2] >= 1).any(), (name, ratio, f.tolist())
        assert nd <= 64 or (f[:, 3] >= 1).any(), (name, ratio, f.tolist())
    node = case(name)[5][2]
    assert (node & ~reference(name, "none", 15)["contested"]).any(), "uncontested nodes exist"


def test_zero_and_none_have_the_same_verdicts_and_confidence():
    for name in ("129-left", "256-right"):
        for ratio in RATIOS:
            a, b = reference(name, "zero", ratio), reference(name, "none", ratio)
            assert a["map"].tobytes() == b["map"].tobytes() and a["conf"].tobytes() == b["conf"].tobytes()
    assert VARIANTS == ("sgm", "zero", "none")


def test_winners_at_both_ends_of_a_lane_row_fail_and_pass():
    """Over the table as a whole: failing and passing winners with jb % 64 == 0 (jb - 1 is lane 63 of the row before) and
    with jb % 64 == 63."""
    seen = set()
    for name, variant, ratio in WITNESSES:
        r = reference(name, variant, ratio)
        for lane in (0, 63):
            at = r["contested"] & (r["jb"] % 64 == lane)
            seen |= {(lane, "fail")} if (at & r["fail"]).any() else set()
            seen |= {(lane, "pass")} if (at & ~r["fail"]).any() else set()
    assert seen == {(0, "fail"), (0, "pass"), (63, "fail"), (63, "pass")}


def test_the_tie_rule_has_a_witness():
    """600-left-levels at P = 0: thousands of contested nodes with m2 == Smin == 0, which pass at every ratio."""
    for ratio in RATIOS:
        r = reference("600-left-levels", "none", ratio)
        tie = r["contested"] & (r["m2"] == 0) & (r["smin"] == 0)
        assert 3500 < int(tie.sum()) < 4300
        assert not (tie & r["fail"]).any()
        assert (r["conf"][tie] == 0).all()
    # ... and with penalties the case fails and passes like the others
    assert figures("600-left-levels", "sgm", 60)[:2] == (1404, 2688)
