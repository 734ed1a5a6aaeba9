"""The table of staircase cases the device tests of the uniqueness ratio run (tests/test_gpu_unique.py), and their
references, computed once per case.  TEST INFRASTRUCTURE ONLY.  tests/test_unique_inputs.py shows on the reference alone
that these cases can tell a wrong winner kernel from a right one."""
import functools

import numpy as np

from sgm_inputs import staircase_case
from sgm_ref import BIG
from unique_ref import sums, unique_from_sums, volume

# cases of sgm_inputs.STAIRCASES.  129-left: 16-bit costs, 32-bit sums; 256-right (its big P2): 32-bit costs, 64-bit sums;
# 2048-left: the whole range a lane can hold, 32 entries each
STAIRCASES = ["129-left", "256-right", "257-left", "seams-left", "2048-left", "600-left-levels"]
RATIOS = (0, 15, 60, 100)
VARIANTS = ("sgm", "zero", "none")   # the case's ws_sgm_params; {paths, 0, 0}; sgm == NULL


@functools.lru_cache(maxsize=None)
def case(name):
    """(L, R, (view, block_size, min_d, max_d, cost), (paths, p1, p2), nd, V) of a staircase case."""
    L, R, (view, bs, mind, maxd, cost, paths, p1, p2), nd, _ = staircase_case(name)
    return L, R, (view, bs, mind, maxd, cost), (paths, p1, p2), nd, volume(L, R, view, bs, mind, maxd, cost)


def sgm_of(name, variant):
    paths, p1, p2 = case(name)[3]
    return {"sgm": (paths, p1, p2), "zero": (paths, 0, 0), "none": None}[variant]


@functools.lru_cache(maxsize=None)
def case_sums(name, variant):
    """S of a case (read only: shared by every ratio).  "zero" is paths * C without walking the paths."""
    V = case(name)[5]
    if variant == "zero":
        S = case_sums(name, "none")
        return np.where(S < BIG, S * case(name)[3][0], BIG)
    return sums(V, sgm_of(name, variant))


def reference(name, variant, ratio, subpixel=False, rivals="rule"):
    L, R, (view, bs, mind, maxd, cost), sgm, nd, V = case(name)
    return unique_from_sums(V, case_sums(name, variant), view, ratio, subpixel, rivals)
