"""The NumPy restatement of the fixed tree (tests/tree_restatement.py) held to what it must be whatever the data: every value counted
once, the lane order a real parameter, the padding +0.0, its constants the header's."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib  # noqa: E402
import tree_restatement as T  # noqa: E402


@pytest.mark.parametrize("order", ["near", "far"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 4096 * 1024 + 5])
def test_ones_sum_to_their_number(n, order):
    """Integers this small add exactly along any tree: the sum is n only if every value is placed, and placed once."""
    assert T.two_level(np.ones((n, 1)), order).tolist() == [float(n)]


def test_the_two_lane_orders_differ():
    x = np.random.default_rng(14).standard_normal((4096 * 3 + 17, 2))
    near, far = T.two_level(x, "near"), T.two_level(x, "far")
    assert (near != far).any() and np.allclose(near, far, rtol=0, atol=1e-9)
    # "far" is the strided halving s[k] += s[k + d], d = 8, 4, 2, 1, operand for operand
    v = np.random.default_rng(15).standard_normal((16, 20000))
    s = v.copy()
    for d in (8, 4, 2, 1):
        s = s[:d] + s[d:2 * d]
    assert np.array_equal(T.lane_tree(v, "far"), s[0]) and int((T.lane_tree(v, "near") != s[0]).sum()) > 1000
    assert T.ORDERS["far"][:6] == [0, 8, 4, 12, 2, 10] and sorted(T.ORDERS["far"]) == T.ORDERS["near"]


def test_the_padding_is_positive_zero():
    for order in ("near", "far"):
        got = T.two_level(np.array([[-0.0]]), order)
        assert got[0] == 0.0 and not np.signbit(got[0])
    # a whole second level of -0.0 partials has no padding to meet: the sign survives, as on the device
    assert np.signbit(T.top_join(np.full(T.TOP, -0.0))) and not np.signbit(T.top_join(np.full(T.TOP - 1, -0.0)))


def test_constants_are_the_headers_and_levels_follow_from_them():
    assert (T.LANES, T.PER, T.TOP) == (lib.header_constant("VFN_TREE_LANES"), lib.header_constant("VFN_TREE_PER"), lib.header_constant("VFN_TREE_TOP"))
    assert T.TILE == lib.REDUCE_TILE and T.TOP == lib.REDUCE_TOP == lib.IMAGE_TOP
    # lane levels + log2(256) + the serial run + log2(1024)
    assert lib.tree_sum_levels(4, 1) == 4 + 8 + 0 + 10 and lib.tree_sum_levels(2, 1025) == 2 + 8 + 1 + 10
    assert lib.tree_sum_levels(0, 1024) == 18 and lib.tree_sum_levels(0, 3 * 1024 + 1) == 21
