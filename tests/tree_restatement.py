"""The fixed tree of include/vfn.h ("The fixed tree": csrc/vfn_tree.h) restated in NumPy, addition for addition, each with the operands
the device gives it in the order it gives them.  NumPy does not reassociate elementwise additions, so the bits are the device's.  The
one restatement of the tree for vfn_reduce_stats (order "far"), vfn_icp_accumulate (order "near") and the image sums (no lane tree:
tests/metrics2d_restatement.py builds its own tiles and uses ``block_tree`` and ``top_join``).  Not part of the package: tests only."""
import numpy as np

LANES, PER, TOP = 256, 16, 1024          # include/vfn.h: VFN_TREE_LANES, VFN_TREE_PER, VFN_TREE_TOP
TILE = LANES * PER
# position -> slot of a lane's 16 values: "near" joins slot k with slot k + 1 first, "far" slot k with slot k + 8 (the 4-bit reversal)
ORDERS = {"near": list(range(PER)), "far": [int(f"{k:04b}"[::-1], 2) for k in range(PER)]}


def block_tree(a):
    """a[B, lanes] -> [B]: lane l takes lane l + d for d = lanes / 2 ... 1, the lower lane on the left."""
    d = a.shape[1] // 2
    assert 2 * d == a.shape[1]
    while d >= 1:
        a = a[:, :d] + a[:, d:2 * d]
        d //= 2
    return a[:, 0]


def top_join(part):
    """part[P] -> the second level: lane l of 1024 starts from partial l (+0.0 if l >= P), adds the partials l + 1024, l + 2048, ...
    serially (a lane adds nothing where there is no partial), then the block tree."""
    n = part.shape[0]
    s = np.zeros(TOP)
    s[:min(n, TOP)] = part[:TOP]
    for k in range(1, -(-n // TOP)):
        chunk = part[k * TOP:(k + 1) * TOP]
        s[:chunk.shape[0]] = s[:chunk.shape[0]] + chunk
    return block_tree(s[None])[0]


def lane_tree(values16, order):
    """values16[16, ...] (a lane's slots along axis 0) -> [...]: the balanced tree over the slots taken in ``order``, neighbouring
    positions first, the lower position on the left — what the device's binary counter builds."""
    a = values16[ORDERS[order]]
    while a.shape[0] > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def two_level(values, order):
    """values[n, C] -> [C]: every column along the two-level tree.  Padded with +0.0 to whole tiles of 4096; value b 4096 + l + 256 k
    sits at (block b, lane l, slot k)."""
    values = np.asarray(values, dtype=np.float64)
    n, c = values.shape
    blocks = -(-n // TILE)
    out = np.empty(c)
    for j in range(c):                                   # column by column: the padded copy of a 4M-row input stays small
        pad = np.zeros(blocks * TILE)
        pad[:n] = values[:, j]
        lanes = lane_tree(pad.reshape(blocks, PER, LANES).transpose(1, 0, 2), order)          # [slot k, b, l] -> [b, l]
        out[j] = top_join(block_tree(lanes))
    return out
