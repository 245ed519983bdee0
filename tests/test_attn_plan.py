"""CPU: the attention dispatch as a table.  attn_plan (csrc/attention.hip) decides every flash-attention launch of the U-Net and text
engines on the host; dh_dbg_attn_plan queries it without a device or a launch.  The rows below are every distinct attention launch of
the SD-2-depth forward + backward passes at batch 1, 2, 8 and 16 (64 x 64 latents), of batch 2 at 96 x 96 latents, of a backward with
the text gradient (the null-text inversion path: cross-attention dK/dV with the engine's split-K workspace as scratch) at batch 1 and
2, and of the text tower's causal forward at batch 1 and 2.  The queries are the ATTNPLAN lines of a tuning build (DH_ATTN_LOG=1,
profiles/attn_plan/attnplan.txt); the pinned values were read off the kernel trace of the same passes with the library of the commit
BEFORE attn_plan existed (profiles/attn_plan/launches.txt: KS, QW and DB from the mangled kernel name; for dK/dV grid x = qchunks when
a k_attn_dkv_reduce follows) -- the 524 plan lines and that trace's attention kernels match one for one.  A threshold edit shows up as
a diff of THIS table.

A row is (query, pinned plan fields).
  query: kind (0 forward, 1 dQ, 2 dK/dV), B, H, Nq, Nk, causal, scratch_elems (f32 elements of dK/dV workspace, 0 = none)
  plan:  ks, qw, db, qchunks, reduce -- the other fields follow from these (check_derived)"""
import ctypes

FWD, DQ, DKV = 0, 1, 2
FIELDS = ("launch", "ks", "qw", "db", "grid_x", "grid_y", "grid_z", "block", "qchunks", "reduce", "scratch_used")
PINNED = ("ks", "qw", "db", "qchunks", "reduce")
LAST = ("ks", "qw", "db", "grid_x", "grid_y", "grid_z", "block", "qchunks", "reduce")      # dh_dbg_attn_last_launch
CUS = 256                      # ATTN_CUS of csrc/unet_kernels.h
DBG_SCRATCH = 16 << 20         # f32 elements dh_dbg_attention hands dK/dV (csrc/debug_api.cpp)

PASSES = {}
# per pass: the launches no earlier pass of this list has
PASSES["unet latent 64 B=1 forward"] = [
    ((0, 1, 5, 4096, 4096, 0, 0), (4, 3, 1, 1, 0)),
    ((0, 1, 10, 1024, 1024, 0, 0), (4, 2, 1, 1, 0)),
    ((0, 1, 20, 256, 256, 0, 0), (2, 1, 1, 1, 0)),
    ((0, 1, 20, 64, 64, 0, 0), (1, 1, 0, 1, 0)),
]
PASSES["unet latent 64 B=1 backward"] = [
    ((1, 1, 5, 4096, 4096, 0, 0), (4, 3, 1, 1, 0)),
    ((2, 1, 5, 4096, 4096, 0, 0), (2, 3, 1, 1, 0)),
    ((1, 1, 10, 1024, 1024, 0, 0), (4, 2, 1, 1, 0)),
    ((2, 1, 10, 1024, 1024, 0, 0), (2, 2, 1, 1, 0)),
    ((1, 1, 20, 256, 256, 0, 0), (2, 1, 1, 1, 0)),
    ((2, 1, 20, 256, 256, 0, 0), (2, 1, 1, 1, 0)),
    ((1, 1, 20, 64, 64, 0, 0), (1, 1, 0, 1, 0)),
    ((2, 1, 20, 64, 64, 0, 0), (1, 1, 1, 1, 0)),
]
# unet latent 64 B=1 forward (text-gradient pass): nothing new
PASSES["unet latent 64 B=1 backward with the text gradient"] = [
    ((1, 1, 5, 4096, 77, 0, 0), (1, 3, 0, 1, 0)),
    ((2, 1, 5, 4096, 77, 0, 335544320), (1, 3, 1, 32, 1)),
    ((1, 1, 10, 1024, 77, 0, 0), (1, 2, 0, 1, 0)),
    ((2, 1, 10, 1024, 77, 0, 335544320), (1, 3, 1, 8, 1)),
    ((1, 1, 20, 256, 77, 0, 0), (1, 1, 0, 1, 0)),
    ((2, 1, 20, 256, 77, 0, 335544320), (2, 1, 1, 1, 0)),
    ((1, 1, 20, 64, 77, 0, 0), (1, 1, 0, 1, 0)),
    ((2, 1, 20, 64, 77, 0, 335544320), (1, 1, 1, 1, 0)),
]
PASSES["unet latent 64 B=2 forward"] = [
    ((0, 2, 5, 4096, 4096, 0, 0), (4, 3, 1, 1, 0)),
    ((0, 2, 10, 1024, 1024, 0, 0), (4, 3, 1, 1, 0)),
    ((0, 2, 20, 256, 256, 0, 0), (2, 2, 1, 1, 0)),
    ((0, 2, 20, 64, 64, 0, 0), (1, 1, 0, 1, 0)),
]
PASSES["unet latent 64 B=2 backward"] = [
    ((1, 2, 5, 4096, 4096, 0, 0), (4, 3, 1, 1, 0)),
    ((2, 2, 5, 4096, 4096, 0, 0), (2, 3, 1, 1, 0)),
    ((1, 2, 10, 1024, 1024, 0, 0), (4, 3, 1, 1, 0)),
    ((2, 2, 10, 1024, 1024, 0, 0), (2, 3, 1, 1, 0)),
    ((1, 2, 20, 256, 256, 0, 0), (2, 2, 1, 1, 0)),
    ((2, 2, 20, 256, 256, 0, 0), (2, 2, 1, 1, 0)),
    ((1, 2, 20, 64, 64, 0, 0), (1, 1, 0, 1, 0)),
    ((2, 2, 20, 64, 64, 0, 0), (1, 1, 1, 1, 0)),
]
# unet latent 64 B=2 forward (text-gradient pass): nothing new
PASSES["unet latent 64 B=2 backward with the text gradient"] = [
    ((1, 2, 5, 4096, 77, 0, 0), (1, 1, 0, 1, 0)),
    ((2, 2, 5, 4096, 77, 0, 335544320), (1, 3, 1, 25, 1)),
    ((1, 2, 10, 1024, 77, 0, 0), (1, 3, 0, 1, 0)),
    ((2, 2, 10, 1024, 77, 0, 335544320), (1, 3, 1, 8, 1)),
    ((1, 2, 20, 256, 77, 0, 0), (1, 2, 0, 1, 0)),
    ((2, 2, 20, 256, 77, 0, 335544320), (2, 1, 1, 1, 0)),
    ((1, 2, 20, 64, 77, 0, 0), (1, 1, 0, 1, 0)),
    ((2, 2, 20, 64, 77, 0, 335544320), (1, 1, 1, 1, 0)),
]
PASSES["unet latent 64 B=8 forward"] = [
    ((0, 8, 5, 4096, 4096, 0, 0), (4, 4, 0, 1, 0)),
    ((0, 8, 5, 4096, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((0, 8, 10, 1024, 1024, 0, 0), (1, 4, 0, 1, 0)),
    ((0, 8, 10, 1024, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((0, 8, 20, 256, 256, 0, 0), (2, 1, 0, 1, 0)),
    ((0, 8, 20, 256, 77, 0, 0), (1, 1, 0, 1, 0)),
    ((0, 8, 20, 64, 64, 0, 0), (1, 2, 0, 1, 0)),
]
PASSES["unet latent 64 B=8 backward"] = [
    ((1, 8, 5, 4096, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((1, 8, 5, 4096, 4096, 0, 0), (2, 4, 0, 1, 0)),
    ((2, 8, 5, 4096, 4096, 0, 0), (2, 4, 1, 1, 0)),
    ((1, 8, 10, 1024, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((1, 8, 10, 1024, 1024, 0, 0), (2, 4, 0, 1, 0)),
    ((2, 8, 10, 1024, 1024, 0, 0), (2, 4, 1, 1, 0)),
    ((1, 8, 20, 256, 77, 0, 0), (1, 1, 0, 1, 0)),
    ((1, 8, 20, 256, 256, 0, 0), (2, 1, 0, 1, 0)),
    ((2, 8, 20, 256, 256, 0, 0), (2, 1, 1, 1, 0)),
    ((1, 8, 20, 64, 64, 0, 0), (1, 2, 0, 1, 0)),
    ((2, 8, 20, 64, 64, 0, 0), (1, 2, 1, 1, 0)),
]
PASSES["unet latent 64 B=16 forward"] = [
    ((0, 16, 5, 4096, 4096, 0, 0), (4, 4, 0, 1, 0)),
    ((0, 16, 5, 4096, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((0, 16, 10, 1024, 1024, 0, 0), (1, 4, 0, 1, 0)),
    ((0, 16, 10, 1024, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((0, 16, 20, 256, 256, 0, 0), (1, 4, 0, 1, 0)),
    ((0, 16, 20, 256, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((0, 16, 20, 64, 64, 0, 0), (1, 1, 0, 1, 0)),
]
PASSES["unet latent 64 B=16 backward"] = [
    ((1, 16, 5, 4096, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((1, 16, 5, 4096, 4096, 0, 0), (2, 4, 0, 1, 0)),
    ((2, 16, 5, 4096, 4096, 0, 0), (2, 4, 1, 1, 0)),
    ((1, 16, 10, 1024, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((1, 16, 10, 1024, 1024, 0, 0), (2, 4, 0, 1, 0)),
    ((2, 16, 10, 1024, 1024, 0, 0), (2, 4, 1, 1, 0)),
    ((1, 16, 20, 256, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((1, 16, 20, 256, 256, 0, 0), (2, 4, 0, 1, 0)),
    ((2, 16, 20, 256, 256, 0, 0), (2, 4, 1, 1, 0)),
    ((1, 16, 20, 64, 64, 0, 0), (1, 1, 0, 1, 0)),
    ((2, 16, 20, 64, 64, 0, 0), (1, 1, 1, 1, 0)),
]
PASSES["unet latent 96 B=2 forward"] = [
    ((0, 2, 5, 9216, 9216, 0, 0), (4, 4, 0, 1, 0)),
    ((0, 2, 5, 9216, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((0, 2, 10, 2304, 2304, 0, 0), (4, 3, 1, 1, 0)),
    ((0, 2, 10, 2304, 77, 0, 0), (1, 3, 0, 1, 0)),
    ((0, 2, 20, 576, 576, 0, 0), (2, 3, 1, 1, 0)),
    ((0, 2, 20, 144, 144, 0, 0), (1, 1, 0, 1, 0)),
    ((0, 2, 20, 144, 77, 0, 0), (1, 1, 0, 1, 0)),
]
PASSES["unet latent 96 B=2 backward"] = [
    ((1, 2, 5, 9216, 77, 0, 0), (1, 4, 0, 1, 0)),
    ((1, 2, 5, 9216, 9216, 0, 0), (2, 4, 0, 1, 0)),
    ((2, 2, 5, 9216, 9216, 0, 0), (2, 4, 1, 1, 0)),
    ((1, 2, 10, 2304, 77, 0, 0), (1, 3, 0, 1, 0)),
    ((1, 2, 10, 2304, 2304, 0, 0), (4, 3, 1, 1, 0)),
    ((2, 2, 10, 2304, 2304, 0, 0), (2, 3, 1, 1, 0)),
    ((1, 2, 20, 576, 576, 0, 0), (2, 3, 1, 1, 0)),
    ((2, 2, 20, 576, 576, 0, 0), (2, 3, 1, 1, 0)),
    ((1, 2, 20, 144, 77, 0, 0), (1, 1, 0, 1, 0)),
    ((1, 2, 20, 144, 144, 0, 0), (1, 1, 0, 1, 0)),
    ((2, 2, 20, 144, 144, 0, 0), (1, 1, 1, 1, 0)),
]
PASSES["text tower B=1"] = [
    ((0, 1, 16, 77, 77, 1, 0), (1, 1, 0, 1, 0)),
]
PASSES["text tower B=2"] = [
    ((0, 2, 16, 77, 77, 1, 0), (1, 1, 0, 1, 0)),
]


def _lib():
    from diffusionhandles_amd import _lib
    return _lib


def plan(kind, B, H, Nq, Nk, causal=0, scratch=0, force_ks=0, force_qw=0, force_dkv_ks=0, force_dkv_qw=0, cus=0):
    L = _lib()
    q = L.AttnPlanQuery(kind, B, H, Nq, Nk, causal, scratch, force_ks, force_qw, force_dkv_ks, force_dkv_qw, cus)
    out = (ctypes.c_int32 * len(FIELDS))()
    L.check(L.lib().dh_dbg_attn_plan(ctypes.byref(q), out, len(FIELDS)), "dh_dbg_attn_plan")
    return tuple(out)


def named(p):
    return dict(zip(FIELDS, p))


def last_launch(kind):
    L = _lib()
    out = (ctypes.c_int32 * len(LAST))()
    L.check(L.lib().dh_dbg_attn_last_launch(kind, out, len(LAST)), "dh_dbg_attn_last_launch")
    return dict(zip(LAST, out))


def rows(names=None):
    for name in names or PASSES:
        yield from PASSES[name]


def cdiv(a, b):
    return -(-a // b)


def check_derived(q, p):
    """the fields the table does not pin follow from the ones it does"""
    kind, B, H, Nq, Nk, causal, scratch = q
    if min(B, H, Nq, Nk) <= 0:
        assert p["launch"] == 0
        return
    assert p["launch"] == 1 and p["block"] == 64 * p["qw"] * p["ks"] and (p["grid_y"], p["grid_z"]) == (H, B)
    assert p["reduce"] == int(p["qchunks"] > 1)
    if kind == DKV:
        assert p["grid_x"] == (p["qchunks"] if p["reduce"] else cdiv(Nk, 32 * p["qw"]))
        assert p["scratch_used"] == (p["qchunks"] * B * H * 2 * 32 * p["qw"] * 64 if p["reduce"] else 0) <= scratch
    else:
        assert p["grid_x"] == cdiv(Nq, 32 * p["qw"]) and p["qchunks"] == 1 and p["scratch_used"] == 0
        assert not p["db"] or (p["ks"] >= 2 and p["ks"] * p["qw"] < 16)
        assert kind != DQ or p["ks"] * p["qw"] != 16
    assert not causal or p["ks"] == 1


def test_attn_plan_table():
    """every distinct launch of the passes gets the pinned plan"""
    n = 0
    for q, want in rows():
        p = named(plan(*q))
        assert tuple(p[f] for f in PINNED) == want, (q, p)
        check_derived(q, p)
        n += 1
    assert n == 96


def test_plan_is_a_function_of_the_query():
    """asking twice, or in another order, gives the same answer"""
    qs = [q for q, _ in rows()]
    first = [plan(*q) for q in qs]
    assert [plan(*q) for q in qs] == first
    assert [plan(*q) for q in reversed(qs)] == first[::-1]


def test_no_launch_exactly_for_a_non_positive_dimension():
    for kind in (FWD, DQ, DKV):
        for i in range(4):
            for bad in (0, -1):
                dims = [2, 5, 1024, 77]
                dims[i] = bad
                p = named(plan(kind, *dims, 0, DBG_SCRATCH))
                assert p["launch"] == 0 and not any(p.values()), (kind, dims, p)
                check_derived((kind, *dims, 0, DBG_SCRATCH), p)
        assert named(plan(kind, 1, 1, 1, 1))["launch"] == 1


def test_rules_flip_at_their_thresholds():
    """both sides of each policy threshold (the constants of csrc/attention.hip)"""
    kq = lambda *a, **k: (lambda p: (p["ks"], p["qw"]))(named(plan(*a, **k)))
    f = lambda *a, **k: named(plan(*a, **k))
    # key split: two wave groups from 4 key tiles on, four from 16 (dK/dV: over the query tiles, at most two)
    for kind in (FWD, DQ):
        assert [f(kind, 1, 20, 64, nk)["ks"] for nk in (192, 193, 256, 960, 961, 1024)] == [1, 2, 2, 2, 4, 4]
    assert [f(DKV, 1, 20, nq, 64)["ks"] for nq in (192, 193, 960, 961, 4096)] == [1, 2, 2, 2, 2]
    # the causal cap: one group whatever the key count
    assert [f(FWD, 1, 16, 77, nk, causal=1)["ks"] for nk in (77, 256, 1024, 4096)] == [1, 1, 1, 1]
    assert f(FWD, 1, 16, 1024, 1024, causal=0)["ks"] == 4
    # the double buffer: key-split blocks of at most 512 workgroups (forward and dQ)
    wg_db = lambda *a, **k: (lambda p: (p["grid_x"] * p["grid_y"] * p["grid_z"], p["ks"] >= 2 and p["ks"] * p["qw"] < 16, p["db"]))(f(*a, **k))
    assert wg_db(DQ, 8, 64, 32, 256) == (512, True, 1) and wg_db(DQ, 9, 57, 32, 256) == (513, True, 0)
    # (the forward: the row-wave rule gives no key-split grid of exactly 513 = 27 x 19 workgroups -- on 513 blocks of one row wave
    #  the big-grid rule has taken the key split away -- so the nearest above, and both sides under a forced row-wave count)
    assert wg_db(FWD, 2, 64, 384, 256) == (512, True, 1) and wg_db(FWD, 7, 37, 64, 256) == (518, True, 0)
    assert wg_db(FWD, 8, 64, 32, 4096, force_qw=1) == (512, True, 1) and wg_db(FWD, 27, 19, 32, 4096, force_qw=1) == (513, True, 0)
    for kind in (FWD, DQ):
        assert wg_db(kind, 1, 8, 2048, 128) == (256, False, 0)                         # one key group: no second buffer
    # the big grid: cdiv(Nq, 128) * H * B >= 512 takes the 128-row block whatever the even-coverage rule says (64 rows: two waves)
    assert kq(FWD, 7, 73, 64, 256) == (2, 2) and kq(FWD, 8, 64, 64, 256) == (1, 4)                       # 511 / 512
    assert kq(DQ, 7, 73, 64, 256) == (2, 2) and kq(DQ, 8, 64, 64, 256) == (2, 4)
    assert f(DKV, 7, 73, 256, 64)["qw"] == 2 and f(DKV, 8, 64, 256, 64)["qw"] == 4
    # ... on which the forward splits no key loop under 64 tiles
    assert kq(FWD, 8, 64, 128, 63 * 64) == (1, 4) and kq(FWD, 8, 64, 128, 63 * 64 + 1) == (4, 4)
    # min_qw: more than 1024 rows in the loop and no 32-row block
    assert kq(FWD, 1, 1, 32, 1024) == (4, 1) and kq(FWD, 1, 1, 32, 1025) == (4, 2)
    assert kq(DQ, 1, 1, 32, 1024) == (4, 1) and kq(DQ, 1, 1, 32, 1025) == (4, 2)
    assert f(DKV, 1, 1, 1024, 32)["qw"] == 1 and f(DKV, 1, 1, 1025, 32)["qw"] == 2
    # dQ has no 16-wave block: (4, 4) becomes (2, 4), also when a tuning build forces both
    assert kq(FWD, 8, 64, 128, 4096) == (4, 4) and kq(DQ, 8, 64, 128, 4096) == (2, 4)
    assert kq(DQ, 1, 5, 4096, 4096) == (4, 3) and kq(DQ, 1, 5, 4096, 4096, force_ks=4, force_qw=4) == (2, 4)
    assert kq(FWD, 1, 5, 4096, 4096, force_ks=4, force_qw=4) == (4, 4)
    # dK/dV's few-key path: at most 128 keys, at least 512 queries, scratch given
    few = lambda nq, nk, scratch=DBG_SCRATCH, **k: f(DKV, 1, 5, nq, nk, 0, scratch, **k)
    assert (few(4096, 128)["qw"], few(4096, 128)["qchunks"]) == (4, 32) and few(4096, 129)["qchunks"] == 1
    assert few(512, 77)["qchunks"] == 4 and few(511, 77)["qchunks"] == 1
    assert few(4096, 77, 0)["qchunks"] == 1 and few(4096, 77, 0)["reduce"] == 0
    # ... the chunks' partials fit the scratch: one element short of 32 chunks gives 31
    need = 32 * 1 * 5 * 2 * 32 * 3 * 64
    assert few(4096, 77, need)["qchunks"] == 32 and few(4096, 77, need)["scratch_used"] == need
    assert few(4096, 77, need - 1)["qchunks"] == 31
    # ... at most one chunk per two query tiles, else the CUs over the (head, image) pairs
    assert few(1024, 77)["qchunks"] == 8 and few(1025, 77)["qchunks"] == 8 and few(1152, 77)["qchunks"] == 9
    assert few(8192, 77)["qchunks"] == CUS // 5 and f(DKV, 2, 5, 8192, 77, 0, DBG_SCRATCH)["qchunks"] == CUS // 10
    assert few(8192, 77, cus=100)["qchunks"] == 20
    for nq in (511, 512, 1024, 4096, 8192):
        for nk in (77, 128, 129):
            q = (DKV, 1, 5, nq, nk, 0, DBG_SCRATCH)
            check_derived(q, named(plan(*q)))


def has(kind, ks, qw, db):
    """the instantiations attention.o holds (AttnFwd / AttnDq / AttnDkv::has of csrc/attention.hip; DH_DKV_DB = 1 in the product)"""
    if ks not in ((1, 2) if kind == DKV else (1, 2, 4)) or not 1 <= qw <= 4:
        return False
    if kind == DKV:
        return db == 1
    return (kind == FWD or ks * qw < 16) and (not db or (ks >= 2 and ks * qw < 16))


def test_every_plan_names_an_instantiation_also_under_forced_values():
    """the launch switch aborts on a plan without an instantiation (no kernel would run): no plan names one, whatever a tuning build
    forces -- in particular dQ's (4, 4), which has no kernel, comes out as (2, 4)"""
    shapes = [(1, 5, 4096, 4096), (1, 5, 4096, 77), (2, 10, 1024, 1024), (8, 20, 256, 256), (16, 5, 4096, 4096), (1, 20, 64, 64),
              (1, 16, 77, 77), (2, 5, 9216, 9216), (1, 1, 32, 1025), (8, 64, 128, 4096), (1, 5, 511, 128), (3, 7, 1000, 129)]
    n = 0
    for kind in (FWD, DQ, DKV):
        for fks in (0, 1, 2, 4):
            for fqw in range(5):
                for dks, dqw in ((0, 0), (1, 1), (2, 4), (1, 3)):
                    for B, H, Nq, Nk in shapes:
                        for scratch in ((0, DBG_SCRATCH) if kind == DKV else (0,)):
                            q = (kind, B, H, Nq, Nk, int(kind == FWD and Nq == 77), scratch)
                            p = named(plan(*q, force_ks=fks, force_qw=fqw, force_dkv_ks=dks, force_dkv_qw=dqw))
                            assert has(kind, p["ks"], p["qw"], p["db"]), (q, fks, fqw, dks, dqw, p)
                            check_derived(q, p)
                            n += 1
    assert n > 3000
    assert has(DQ, 2, 4, 1) and not has(DQ, 4, 4, 0) and not has(FWD, 4, 4, 1) and has(FWD, 4, 4, 0) and not has(DKV, 4, 1, 1)


# ---- the variants the GPU parity test launches (tests/test_unet_kernels_gpu.py: test_attention_forward_backward) -----------------------
# (B, H, Nq, Nk) of that test; dh_dbg_attention runs forward, dQ and dK/dV (with DBG_SCRATCH) on each
PARITY_SHAPES = [(1, 5, 1024, 1024), (2, 2, 256, 256), (1, 20, 64, 64), (2, 5, 1024, 77), (1, 10, 200, 77), (1, 5, 4096, 77),
                 (1, 2, 4096, 4096), (1, 3, 1000, 1000), (1, 2, 1100, 600)]
# added so that every (kind, ks, qw, db) of the table is launched
VARIANT_SHAPES = [(1, 20, 256, 256), (8, 20, 256, 256), (2, 20, 256, 256), (1, 10, 1024, 1024), (4, 20, 200, 200), (4, 20, 200, 1024),
                  (16, 20, 200, 200), (4, 20, 320, 32), (8, 20, 64, 64), (1, 5, 13200, 4096)]
# variants of PARITY_SHAPES that no engine pass of the table launches (B = 1, H <= 5, about 1000 rows: 32-row blocks, four key groups)
NOT_IN_TABLE = {(FWD, 4, 1, 1), (DQ, 4, 1, 1)}


def variants(B, H, Nq, Nk):
    out = set()
    for kind in (FWD, DQ, DKV):
        p = named(plan(kind, B, H, Nq, Nk, 0, DBG_SCRATCH if kind == DKV else 0))
        out.add((kind, p["ks"], p["qw"], p["db"]))
    return out


def test_parity_shapes_launch_exactly_the_variants_of_the_table():
    table = set()
    for q, want in rows():
        table.add((q[0],) + want[:3])
    launched = set().union(*(variants(*s) for s in PARITY_SHAPES + VARIANT_SHAPES))
    print(f"{len(table)} variants in {sum(1 for _ in rows())} rows")
    assert len(table) == 29
    assert launched - table == NOT_IN_TABLE and table - launched == set(), (sorted(table - launched), sorted(launched - table))
    assert set().union(*(variants(*s) for s in VARIANT_SHAPES)) <= table
    # the text tower's causal launch cannot go through dh_dbg_attention (no causal argument): its variant through the query only
    p = named(plan(FWD, 1, 16, 77, 77, causal=1))
    assert (FWD, p["ks"], p["qw"], p["db"]) in table and p["ks"] == 1


# (B, H, N) with Nq = Nk = N of the causal parity test (tests/test_engine_kernels_gpu.py: test_attention_causal, through
# dh_dbg_attention_causal): the text tower's two launches, one partial tile, both sides of a 64-key tile edge, three tiles with a ragged
# last one, and 576 rows at two batch sizes (nine key tiles, most of them hidden from the first rows)
CAUSAL_SHAPES = [(1, 16, 77), (2, 16, 77), (1, 4, 20), (1, 2, 64), (1, 2, 65), (1, 3, 129), (1, 16, 576), (4, 16, 576)]


def test_causal_parity_shapes_plan_one_key_group_and_two_block_sizes():
    """a causal launch never splits the keys (a wave group whose keys all lie behind a row would merge m = -inf), and the shapes of the
    parity test run the mask under at least two row-wave counts"""
    plans = []
    for B, H, N in CAUSAL_SHAPES:
        q = (FWD, B, H, N, N, 1, 0)
        p = named(plan(*q))
        check_derived(q, p)
        assert p["launch"] == 1 and p["ks"] == 1 and p["db"] == 0, (q, p)
        plans.append(p)
    assert len({p["qw"] for p in plans}) >= 2, [p["qw"] for p in plans]
