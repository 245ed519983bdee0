"""CPU: the VAE's geometry cases, and the arithmetic its row counts lean on.

tests/test_gemm_classes.py holds the SMALLEST query of every launch class, which loses what is particular to the VAE engine
(csrc/vae_engine.cpp): one image of 512^2 or 768^2 rows.  GEOMETRY_CASES keep the image side and take the fewest channels (multiples
of 64) that still plan into the launch class of the engine's own launch; tests/test_vae_geometry_gpu.py runs them against torch.
Here, without a device:
  - every case plans (dh_dbg_gemm_plan, shipped hooks, the engine's workspace) into the class of the row of tests/test_gemm_plan.py it
    names, and that row is in the table (the arrangement of PARITY_SHAPES in tests/test_attn_plan.py);
  - div_small (csrc/common.h), as the kernels use it at these sizes, in float32 with a reciprocal one ulp off either way: the row /
    column split of the convolutions (589 824 rows over a width of 768) and the slice edges of the GroupNorm statistics kernels
    (HW * s up to 18.9 M over S = 32);
  - a float32 model of the statistics scheme (32 slices, sums shifted by the slice's first element, Chan's merge) on the data of the
    GPU test -- N(0.5, 2) with 4096 in the image's last row -- stays far inside the gates that test sets (|mean error| <= 4096 / (8 HW),
    rstd within 1e-3), while losing the last row, or reading the row behind it, lands far outside: the gates can tell."""
import numpy as np
import pytest

from test_gemm_classes import launch_class
from test_gemm_plan import ALIGNED, BIAS, PASS_PART, PASSES, RESIDUAL, named, plan, shipped_hooks  # noqa: F401  (autouse: the shipped policy)


def conv_q(side, cin, cout, stride=1, up=0, flags=ALIGNED | BIAS):
    out = side * (2 if up else 1) // stride
    return (out * out, cout, 9 * cin, 1, side, stride, up, 0, 0, flags)


def dense_q(M, N, K, flags=ALIGNED | BIAS):
    return (M, N, K, 0, 0, 1, 0, 0, 0, flags)


RES = ALIGNED | BIAS | RESIDUAL
# id -> (query, pad, pass of the plan table, the engine's row there).  The workspace of a case is the pass's (PASS_PART).
GEOMETRY_CASES = {
    # a. stride-1 3x3 (a resnet's conv2, with its residual): 256 persistent workgroups walk 1024 / 2304 / 256 tiles of 256 x 128
    "a-s1-512": (conv_q(512, 64, 128, flags=RES), 1, "vae_dec_lat64", (262144, 128, 1152, 1, 512, 1, 0, 0, 0, 4099)),
    "a-s1-768": (conv_q(768, 64, 128, flags=RES), 1, "vae_dec_lat96", (589824, 128, 1152, 1, 768, 1, 0, 0, 0, 4099)),
    "a-s1-256": (conv_q(256, 64, 128, flags=RES), 1, "vae_dec_lat64", (65536, 256, 2304, 1, 256, 1, 0, 0, 0, 4099)),
    # b. nearest-2x up-sampling fused into the gather
    "b-up-128": (conv_q(128, 64, 128, up=1), 1, "vae_dec_lat64", (65536, 512, 4608, 1, 128, 1, 1, 0, 0, 4097)),
    "b-up-256": (conv_q(256, 64, 128, up=1), 1, "vae_dec_lat64", (262144, 256, 2304, 1, 256, 1, 1, 0, 0, 4097)),
    "b-up-384": (conv_q(384, 64, 128, up=1), 1, "vae_dec_lat96", (589824, 256, 2304, 1, 384, 1, 1, 0, 0, 4097)),
    # c. the encoder's down-sampler: stride 2, zero padding bottom / right only (pad 0); pad 1 at 512 tells a pad bug from a gather
    # bug.  Side 256 leaves 16384 rows: 128 output channels would fall off k_gemm_pp, the engine's 256 keep its 128 x 128 tile.
    "c-s2-512": (conv_q(512, 64, 128, stride=2), 0, "vae_enc_lat64", (65536, 128, 1152, 1, 512, 2, 0, 0, 0, 4097)),
    "c-s2-768": (conv_q(768, 64, 128, stride=2), 0, "vae_enc_lat96", (147456, 128, 1152, 1, 768, 2, 0, 0, 0, 4097)),
    "c-s2-256": (conv_q(256, 64, 256, stride=2), 0, "vae_enc_lat64", (16384, 256, 2304, 1, 256, 2, 0, 0, 0, 4097)),
    "c-s2-512-pad1": (conv_q(512, 64, 128, stride=2), 1, "vae_enc_lat64", (65536, 128, 1152, 1, 512, 2, 0, 0, 0, 4097)),
    # d. a resnet's 1x1 shortcut: a dense GEMM over the image's rows
    "d-1x1-512": (dense_q(262144, 128, 128), 1, "vae_dec_lat64", (262144, 128, 256, 0, 0, 1, 0, 0, 0, 4097)),
    # e. the split forms, at the engine's own shapes
    "e-split-s1-64": (conv_q(64, 512, 512, flags=RES), 1, "vae_dec_lat64", (4096, 512, 4608, 1, 64, 1, 0, 0, 0, 4099)),
    "e-split-s2-128": (conv_q(128, 512, 512, stride=2), 0, "vae_enc_lat64", (4096, 512, 4608, 1, 128, 2, 0, 0, 0, 4097)),
    "e-split-pv": (dense_q(4096, 512, 4096, flags=ALIGNED), 1, "vae_dec_lat64", (4096, 512, 4096, 0, 0, 1, 0, 0, 0, 4096)),
}
# g. the cases that also run on a coordinate ramp with a tap-copying weight (exact in 16 bits: equality)
RAMP_CASES = ("a-s1-768", "b-up-384", "c-s2-768")
# the launch class each group stands for (pp, bm, bn, stages, kg, mw, gm, buf, lnf, epi, split, gn_epi, reduce)
CLASS_OF = {"a": (1, 256, 128, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0), "b": (1, 256, 128, 0, 0, 0, 2, 1, 0, 0, 0, 0, 0),
            "c": (1, 256, 128, 0, 0, 0, 2, 1, 0, 0, 0, 0, 0), "d": (1, 256, 128, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0)}
SPLIT_CLASS = {"e-split-s1-64": (1, 256, 128, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1), "e-split-s2-128": (1, 256, 128, 0, 0, 0, 2, 1, 0, 0, 1, 0, 1),
               "e-split-pv": (1, 256, 128, 0, 0, 0, 0, 1, 0, 0, 1, 0, 1), "c-s2-256": (1, 128, 128, 0, 0, 0, 2, 1, 0, 0, 0, 0, 0)}


def full(q, part):
    return q + (0,) * (16 - len(q)) + (part,)


def case_query(name):
    """the 17-value query of a case: its shape with the workspace of the engine pass it stands for"""
    q, _, pas, _ = GEOMETRY_CASES[name]
    return full(q, PASS_PART[pas])


@pytest.mark.parametrize("name", list(GEOMETRY_CASES))
def test_case_plans_into_the_class_of_its_engine_row(name):
    q, pad, pas, row = GEOMETRY_CASES[name]
    assert row in [r for r, _ in PASSES[pas]], (name, "names a row the table does not have")
    p_case, p_row = named(plan(*case_query(name))), named(plan(*full(row, PASS_PART[pas])))
    assert launch_class(p_case) == launch_class(p_row), (name, p_case, p_row)
    assert launch_class(p_case) == SPLIT_CLASS.get(name, CLASS_OF.get(name[0])), (name, p_case)
    assert p_case["splits"] == p_row["splits"] and (name[0] != "e" or p_case["splits"] == 4), (name, p_case, p_row)
    # the side is the engine's: same rows, same image, so the same tiles walk the same row indices
    assert q[0] == row[0] and q[3:7] == row[3:7] and q[9] == row[9], (name, q, row)
    assert pad == (0 if (row[5] == 2 and name[-4:] != "pad1") else 1)


def test_cases_take_the_fewest_channels_of_their_class():
    """64 fewer input or output channels and the launch is of another class (or cannot be asked for)"""
    for name, (q, _, pas, _) in GEOMETRY_CASES.items():
        if name[0] == "e":
            continue            # (the engine's own shapes)
        want = launch_class(named(plan(*case_query(name))))
        M, N, K = q[:3]
        step = 9 * 64 if q[3] else 64
        # (d keeps K = 128, the engine's shortest shortcut: a K loop of two tiles; one tile would plan the same and loop less)
        for n, k in ((N - 64, K),) + (((N, K - step),) if name[0] != "d" else ()):
            if n >= 64 and k >= step:
                assert launch_class(named(plan(*full((M, n, k) + q[3:], PASS_PART[pas])))) != want, (name, n, k)


# ---- div_small at the VAE's sizes ---------------------------------------------------------------------------------------------------
def div_small(m, inv):
    """csrc/common.h: (int)(((float)m + 0.5f) * inv), in float32"""
    return ((m.astype(np.float32) + np.float32(0.5)) * np.float32(inv)).astype(np.int64)


def rcp_within_one_ulp(d):
    r = np.float32(1.0) / np.float32(d)
    return sorted({float(np.nextafter(r, np.float32(0))), float(r), float(np.nextafter(r, np.float32(2)))})


@pytest.mark.parametrize("side", [512, 768, 384, 256])
def test_div_small_splits_every_row_index_of_an_image(side):
    """row m of one image -> (y, x) = (m / side, m % side), and image index m / side^2 = 0: exact for every m with any reciprocal
    within one ulp (v_rcp_f32's bound)"""
    m = np.arange(side * side, dtype=np.int64)
    for inv in rcp_within_one_ulp(side):
        assert np.array_equal(div_small(m, inv), m // side), (side, inv)
    for inv in rcp_within_one_ulp(side * side):
        assert not div_small(m, inv).any(), (side, inv)
    # two images (the U-Net's batched passes stay below 2^21 rows): the last rows of the first, the first of the second
    edge = np.arange(side * side - 4096, side * side + 4096, dtype=np.int64)
    for inv in rcp_within_one_ulp(side * side):
        assert np.array_equal(div_small(edge, inv), edge // (side * side)), (side, inv)


@pytest.mark.parametrize("HW", [262144, 589824, 65536, 147456])
def test_div_small_gives_the_slice_edges_of_the_statistics_kernels(HW):
    """r0 = div_small(HW * s, 1 / S), S = 32: HW * s reaches 2^23 (512^2) and 18.9 M (768^2), past the 2^22 the general argument covers and,
    at 768^2, past 2^24 where float32 no longer holds every integer.  It comes out right because S is a power of two (its reciprocal
    is exact, and v_rcp_f32 returns it exactly) and HW * s is a multiple of 4096 < 2^24 * 4096, hence a float32; the + 0.5 is then
    either exact or rounded away.  A reciprocal one ulp off would NOT do: that is asserted too, so that nobody widens S to 24."""
    S = 32
    s = np.arange(S + 1, dtype=np.int64)
    assert np.array_equal(div_small(HW * s, 1.0 / S), HW * s // S)
    assert (HW * s // S)[-1] == HW
    lo, _, hi = rcp_within_one_ulp(S)
    both = np.array_equal(div_small(HW * s, lo), HW * s // S) and np.array_equal(div_small(HW * s, hi), HW * s // S)
    assert both == (HW * S < 1 << 23), "a reciprocal one ulp off is survived below 2^23 only"


# ---- the statistics scheme in float32 -------------------------------------------------------------------------------------------------
def to16(x, kind):
    """round float32 to fp16 / bf16 (nearest even) and back"""
    if kind == "fp16":
        return x.astype(np.float16).astype(np.float32)
    b = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def sliced_stats(x, S=32, r0=0, r1=None):
    """(mean, M2 / n) of x [rows][cpg] over rows [r0, r1) the way k_gn_partial + gn_combine get them: per slice f32 sums of x - pivot
    (the slice's first element), (n, mean, M2) per slice, Chan's merge; float32 throughout"""
    f = np.float32
    rows = x.shape[0] if r1 is None else r1
    n_t, m_t, q_t = f(0), f(0), f(0)
    for s in range(S):
        a, b = r0 + (rows - r0) * s // S, r0 + (rows - r0) * (s + 1) // S
        blk = x[a:b].astype(f)
        piv = blk[0, 0]
        d = blk - piv
        sa, sq, n = d.sum(dtype=f), (d * d).sum(dtype=f), f(blk.size)
        mean, m2 = f(piv + sa / n), f(sq - sa * sa / n)
        if n_t == 0:
            n_t, m_t, q_t = n, mean, m2
        else:
            tot, dl = f(n_t + n), f(mean - m_t)
            q_t = f(q_t + m2 + dl * dl * n_t * n / tot)
            m_t = f(m_t + dl * n / tot)
            n_t = tot
    return float(m_t), float(q_t / n_t)


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
@pytest.mark.parametrize("HW", [262144, 589824])
def test_statistics_gates_tell_a_lost_last_row(HW, kind):
    """the data of the GPU test (one group of C = 128, G = 32: four channels): the model's own error against float64, and what an r1 one
    row short, or one row long (into the -4096 row behind the view), does"""
    cpg, eps = 4, 1e-6
    rng = np.random.default_rng(HW + len(kind))
    buf = to16((rng.standard_normal((HW + 1, cpg)) * 2 + 0.5).astype(np.float32), kind)
    buf[HW - 1] = 4096.0
    buf[HW] = -4096.0
    x = buf[:HW]
    mean64, var64 = x.astype(np.float64).mean(), x.astype(np.float64).var()
    rstd64 = 1 / np.sqrt(var64 + eps)
    gate = 4096.0 / (8 * HW)
    mean, var = sliced_stats(x)
    em, er = abs(mean - mean64), abs(1 / np.sqrt(var + eps) / rstd64 - 1)
    print(f"HW {HW} {kind}: model mean error {em:.2e} (gate {gate:.2e}), rstd {er:.2e} (gate 1e-3)")
    assert em < gate / 8 and er < 1e-3 / 8
    for what, r1 in (("one row short", HW - 1), ("one row long", HW + 1)):
        m, v = sliced_stats(buf, r1=r1)
        dm, fr = abs(m - mean64), 1 / np.sqrt(v + eps) / rstd64
        print(f"    {what}: mean off by {dm:.2e}, rstd by a factor of {fr:.2f}")
        assert dm > 2 * gate, (what, dm, gate)
        assert fr > 1.5 or fr < 0.8, (what, fr)
