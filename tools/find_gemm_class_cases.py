#!/usr/bin/env python3
"""CPU only: the smallest query of every GEMM launch class of the pinned plan table (tests/test_gemm_plan.py), printed as the
CLASS_CASES table of tests/test_gemm_classes.py.  Run it after a policy edit and paste its output over the table.

A launch class is what differs between two launches (launch_class in tests/test_gemm_classes.py): the arm of launch_planned's
switch, the A-operand form, the epilogue, the riders and the launch after a split.  For each class the search starts from the
table's smallest row of the class (by M N K, the first of equals) and shrinks it by coordinate descent while dh_dbg_gemm_plan
still answers the same class: the split-K workspace, the images, the rows per image (dense) or the input side (convolutions),
K, N and the GEGLU seam, each to the smallest admissible value with the others held, in every order of the four shape coordinates,
until nothing moves; the cheapest end point wins (M N K, then the workspace, then M + N + K; ties: the first order).  Admissible values:
  N, K (dense), Cin (convolutions), the GEGLU seam: multiples of 64 (N of a GEGLU: of 128); N of a cross-attention: 64 per head
  rows per image: multiples of 64, or the row's own count; M is images x rows per image, so M % gn_HW == 0 and M % xa_Nq == 0
  input side of a convolution: multiples of 4 that leave an output of 8 x 8 or more (the deepest level of the engines)
  workspace: 0 or a power of two from 2^16 f32 elements
lda and ldc are the default pitches (the column-split GEGLU backward: ldc = N - seam, the width of its plain output)."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gemm_plan as T  # noqa: E402
from test_gemm_classes import launch_class  # noqa: E402

GN = T.GN_STATS
XA = T.XATTN_FWD | T.XATTN_DQ
GLU = T.GLU_FWD | T.GLU_BWD


def out_side(conv, hw, stride, up):
    return 2 * hw if conv == 2 else hw * (2 if up else 1) // stride


def to_point(q):
    """table row -> the coordinates the search moves: images, rows per image (dense) or input side (conv), N, K or Cin, seam, workspace"""
    M, N, K, conv, hw, stride, up, _, _, flags, gn_HW, _, glub_f, xa_Nq = q[:14]
    per = out_side(conv, hw, stride, up) ** 2 if conv else (gn_HW if flags & GN else (xa_Nq if flags & XA else M))
    assert M % per == 0, q
    return {"B": M // per, "R": hw if conv else per, "N": N, "K": K // 9 if conv else K, "F": glub_f, "part": q[16]}


def to_query(q, pt):
    """... and back, the row's other fields kept"""
    conv, hw, stride, up, flags = q[3], q[4], q[5], q[6], q[9]
    per = out_side(conv, pt["R"], stride, up) ** 2 if conv else pt["R"]
    return (pt["B"] * per, pt["N"], pt["K"] * (9 if conv else 1), conv, pt["R"] if conv else 0, stride, up, 0,
            pt["N"] - pt["F"] if pt["F"] else 0, flags, per if flags & GN else 0, q[11], pt["F"], per if flags & XA else 0, q[14],
            pt["N"] // 64 if flags & XA else 0, pt["part"])


def candidates(q, pt, dim):
    conv, stride, flags = q[3], q[5], q[9]
    top = pt[dim]
    if dim == "B":
        return range(1, top + 1)
    if dim == "R":
        if conv:      # (no output smaller than the 8 x 8 latents of the deepest level)
            return [hw for hw in range(4, top + 1, 4) if out_side(conv, hw, stride, q[6]) >= 8]
        return sorted(set(range(64, top + 1, 64)) | {top})
    if dim == "N":
        step = 128 if flags & GLU and not pt["F"] else 64
        return [n for n in range(step, top + 1, step) if n > pt["F"]]
    if dim == "K":
        return range(64, top + 1, 64)
    if dim == "F":
        return range(64, top + 1, 64) if top else [0]
    return [0] + [1 << s for s in range(16, 40) if 1 << s < top] + [top]


def cost(query):
    M, N, K = query[:3]
    return (M * N * K, query[16], M + N + K)


def shrink(q, cls):
    start = to_point(q)
    assert launch_class(T.named(T.plan(*to_query(q, start)))) == cls, (q, "the default pitches change the class")
    best = None
    for order in (("part",) + o + ("F",) for o in itertools.permutations(("B", "R", "K", "N"))):
        pt = dict(start)
        moved = True
        while moved:
            moved = False
            for dim in order:
                for v in candidates(q, pt, dim):
                    if v >= pt[dim]:
                        break
                    if launch_class(T.named(T.plan(*to_query(q, dict(pt, **{dim: v}))))) == cls:
                        pt[dim] = v
                        moved = True
                        break
        query = to_query(q, pt)
        if best is None or cost(query) < cost(best):
            best = query
    return best


def shipped_policy():
    """the dispatch's process-wide test hooks at their defaults (what the shipped_hooks fixture of tests/test_gemm_plan.py does)"""
    lib = T._lib()
    for fn, v in (("dh_dbg_gemm_family", 0), ("dh_dbg_gemm_stage", 1), ("dh_dbg_gemm_pp_glu", -1), ("dh_dbg_gemm_pp_persist", 1)):
        lib.check(getattr(lib.lib(), fn)(v), fn)


def find_cases():
    """[(class, smallest query)] in the order of the classes' first rows in the table"""
    shipped_policy()
    first = {}
    for q, _ in T.rows():
        cls = launch_class(T.named(T.plan(*q)))
        if cls not in first or q[0] * q[1] * q[2] < first[cls][0] * first[cls][1] * first[cls][2]:
            first[cls] = q
    return [(cls, shrink(q, cls)) for cls, q in first.items()]


def render(cases):
    return "CLASS_CASES = [\n" + "".join(f"    ({cls}, {query}),\n" for cls, query in cases) + "]"


if __name__ == "__main__":
    print(render(find_cases()))
