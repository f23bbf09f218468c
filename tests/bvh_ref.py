"""Reference boxes of a downloaded BVH4 (OptixRenderer.bvh_arrays), in numpy float32: what every
child slot of every node must store for the node links and leaf-ordered triangle records given.
Shared by the GPU tests that check stored boxes bit for bit."""
import numpy as np

EMPTY = np.int32(-0x80000000)  # kEmptyChild


def _f32(words):
    return np.ascontiguousarray(words).view(np.float32)


def _pad(x):
    # pt_device.h box_pad, in float32 without contraction
    return np.abs(x) * np.float32(9.5367431640625e-7) + np.float32(1e-6)


def tri_boxes_padded(recs):
    """pt_device.h tri_box_padded of every leaf-ordered record, in numpy float32."""
    f = _f32(recs)
    a, b, c = f[:, 0:3], f[:, 4:7], f[:, 8:11]
    p1, p2 = a + b, a + c
    lo = np.minimum(np.minimum(a, p1), p2)
    hi = np.maximum(np.maximum(a, p1), p2)
    return lo - _pad(lo), hi + _pad(hi)


def expected_child_boxes(nodes, recs):
    """For every node, the (4, 3) lo / hi boxes its children must store: the union of the padded
    boxes of the triangles below each child; empty slots inverted and infinite."""
    tlo, thi = tri_boxes_padded(recs)
    child = nodes[:, 24:28].view(np.int32)
    memo = {}

    def node_box(n):
        if n not in memo:
            lo = np.full((4, 3), np.inf, np.float32)
            hi = np.full((4, 3), -np.inf, np.float32)
            for k in range(4):
                c = int(child[n, k])
                if c == int(EMPTY):
                    continue
                if c < 0:
                    first, cnt = (~c) >> 3, ((~c) & 7) + 1
                    lo[k], hi[k] = tlo[first:first + cnt].min(axis=0), thi[first:first + cnt].max(axis=0)
                else:
                    clo, chi = node_box(c)
                    lo[k], hi[k] = clo.min(axis=0), chi.max(axis=0)
            memo[n] = (lo, hi)
        return memo[n]

    return [node_box(n) for n in range(len(nodes))]


def stored_child_boxes(nodes, n):
    f = _f32(nodes[n])
    lo = np.stack([f[0:4], f[8:12], f[16:20]], axis=1)
    hi = np.stack([f[4:8], f[12:16], f[20:24]], axis=1)
    return lo, hi
