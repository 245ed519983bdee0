"""CPU: the attention range cases (tests/attention_range.py) before a kernel sees them.

(a) A float64 model of the kernels' two roundings -- P to 16 bits before its product, o to 16 bits before delta, dS to 16 bits
    before its two products, every output once -- passes the gates of test_attention_forward_backward on every family and shape
    with room to spare (at most 0.8 of tolerance, no element over).  So a kernel that misses a gate on the GPU does something the
    model does not: the cases cannot fail through 16-bit storage alone.  A model that flushes fp16 subnormal probabilities misses
    the sink case by several tolerances: the case has teeth.
(b) Through dh_dbg_attn_plan, the launches the shapes of tests/test_attention_range_gpu.py reach: every key-split count with and
    without the double buffer, ragged and whole last tiles, both dK/dV group counts and the few-key reduce."""
import math

import pytest
import torch

import attention_range as R
import test_attn_plan as T
from test_unet_kernels_gpu import close

DTYPES = [torch.float16, torch.bfloat16]
ATTN_TOL = {torch.float16: 5e-3, torch.bfloat16: 3e-2}         # test_attention_forward_backward: forward; dq, dk, dv at twice that
MODEL_ROOM = 0.8
CPU = torch.device("cpu")


def plans(B, H, Nq, Nk):
    """kind -> the plan of dh_dbg_attention's launch of that kind"""
    return {kind: T.named(T.plan(kind, B, H, Nq, Nk, 0, T.DBG_SCRATCH if kind == T.DKV else 0)) for kind in (T.FWD, T.DQ, T.DKV)}


def key_groups(Nk, ks):
    """first key of each wave group's key range (k_attn_fwd / k_attn_bwd_dq: group g owns tiles [g, g + 1) * ceil(tiles / ks))"""
    tiles = T.cdiv(Nk, 64)
    tps = T.cdiv(tiles, ks)
    return [g * tps * 64 for g in range(ks) if g * tps * 64 < Nk]


def group_starts(B, H, Nq, Nk):
    """the keys a key group of the forward's or dQ's plan starts on, the first group's aside: what one_hot places winners around"""
    p = plans(B, H, Nq, Nk)
    return sorted({s for kind in (T.FWD, T.DQ) for s in key_groups(Nk, p[kind]["ks"])[1:]})


def gated(got, ref, dtype, what, log):
    """the outputs through close() at the gates of test_attention_forward_backward; returns {output: worst ratio} as close() logged it"""
    tol = ATTN_TOL[dtype]
    log.write_text("")
    close(got["o"], ref["o"], tol, tol, what + " fwd")
    close(got["lse"], ref["lse"], 1e-3, 2e-3, what + " lse")
    for nm in ("dq", "dk", "dv"):
        close(got[nm], ref[nm], 2 * tol, 2 * tol * max(1.0, ref[nm].abs().max().item()) * 0.2, what + " " + nm)
    ratios = [float(line.split("\t")[-1]) for line in log.read_text().splitlines()]
    assert len(ratios) == 5
    return dict(zip(("o", "lse", "dq", "dk", "dv"), ratios))


def cases():
    return [(s, f) for s in R.SHAPES for f in R.flash_families(s[3]) + ["one_hot"]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,family", cases())
def test_rounding_model_passes_the_gates_with_room(dtype, shape, family, tmp_path, monkeypatch):
    log = tmp_path / "ratios.txt"
    monkeypatch.setenv("DH_CLOSE_RATIOS", str(log))
    c = R.make(family, dtype, *shape, CPU, group_starts=group_starts(*shape))
    got = R.model(c["q"], c["k"], c["v"], c["do"], c["H"], dtype)
    ratios = gated(got, c["ref"], dtype, f"model {family} {dtype} {shape}", log)
    print(f"model {family} {dtype} {shape}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= MODEL_ROOM, ratios


def test_flushed_subnormals_miss_the_sink_case(tmp_path, monkeypatch):
    """fp16, 1099 flat keys 10 nats under the sink: each flat probability is exp(-10) = 4.5e-5 of the row maximum, below fp16's
    smallest normal number 6.1e-5.  Flushed, the forward loses their V while the row sum keeps them: every element of o is off by
    a / (1 + a) = 0.0475, a = 1099 exp(-10), against a tolerance 5e-3 (1 + |o|) -- several tolerances on every element."""
    shape = (1, 2, 320, 1100)
    monkeypatch.setenv("DH_CLOSE_RATIOS", str(tmp_path / "ratios.txt"))
    c = R.make("sink", torch.float16, *shape, CPU)
    got = R.model(c["q"], c["k"], c["v"], c["do"], c["H"], torch.float16, flush_subnormal=True)
    tol = ATTN_TOL[torch.float16]
    ratio = (got["o"] - c["ref"]["o"]).abs() / (tol + tol * c["ref"]["o"].abs())
    print(f"flushed model, sink {shape}: forward ratio min {ratio.min().item():.2f} median {ratio.median().item():.2f} max {ratio.max().item():.2f}")
    a = 1099 * math.exp(-10.0)
    assert ratio.min().item() > 1.0 and ratio.max().item() > 0.9 * (a / (1 + a)) / tol
    with pytest.raises(AssertionError):
        close(got["o"], c["ref"]["o"], tol, tol, "flushed model")


def test_families_are_what_they_say():
    shape = (1, 2, 320, 1100)
    B, H, Nq, Nk = shape
    for dtype in DTYPES:
        mk = lambda f: R.make(f, dtype, *shape, CPU, group_starts=group_starts(*shape))
        c = mk("scaled16")
        top = R.logits(c["q"], c["k"], H).abs().max().item()
        print(f"scaled16 {dtype}: largest |logit| {top:.1f}")
        assert 60 < top < 130
        c = mk("shifted")
        s = R.logits(c["q"], c["k"], H)
        assert s.mean().item() > 50 and c["ref"]["lse"].abs().min().item() > 30
        c = mk("uniform")
        assert torch.allclose(c["ref"]["lse"], torch.full_like(c["ref"]["lse"], R.uniform_lse(Nk)), rtol=1e-14, atol=0)
        mean = R.unheads(R.heads(c["v"].double(), H).mean(dim=2, keepdim=True).expand(B, H, Nq, 64))
        assert torch.allclose(c["ref"]["o"], mean, rtol=0, atol=1e-14)
        c = mk("sink")
        s = R.logits(c["q"], c["k"], H)
        assert sorted(s.unique().tolist()) == [0.0, 10.0] and bool(((s == 10.0).sum(-1) == 1).all())
        for b in range(B):
            for h in range(H):
                assert bool((s[b, h, :, R.sink_key(b, h, Nk)] == 10.0).all())
        c = mk("one_hot")
        s = R.logits(c["q"], c["k"], H)
        assert sorted(s.unique().tolist()) == [0.0, R.ONE_HOT_LOGIT]
        w = R.winners(c)
        assert bool((w.sum(-1) == 1).all()) and torch.equal(w.long().argmax(-1), c["winner"])
        for t in (c["v"], c["do"]):
            assert bool((t.double() == t.double().round()).all()) and t.abs().max().item() == 2
        vw = torch.gather(R.heads(c["v"].double(), H), 2, c["winner"][..., None].expand(B, H, Nq, 64))
        assert (c["ref"]["o"] - R.unheads(vw)).abs().max().item() < 1e-25
        assert (c["ref"]["lse"] - R.ONE_HOT_LOGIT).abs().max().item() < 1e-12
        assert max(c["ref"][n].abs().max().item() for n in ("dq", "dk")) < 1e-25
    for B, H, N in R.CAUSAL_SHAPES:
        c = R.one_hot_causal(torch.bfloat16, B, H, N, CPU)
        w = R.winners(c, causal=True)
        i = torch.arange(N)
        assert torch.equal(w.sum(-1), (i // 64 + 1).expand(B, H, N)) and bool(w[:, :, i, i].all())


def test_one_hot_places_winners_where_the_plan_has_its_edges():
    """the designated keys of every shape: keys 0, 31, 32, 63, 64; both sides of each boundary between two key groups of the forward's
    and dQ's plan; Nk - 1; a key in every group; and the 32 rows of any wave win keys of several tiles and of every key group"""
    for shape in R.SHAPES:
        B, H, Nq, Nk = shape
        starts = group_starts(*shape)
        order = R.designated_keys(Nk, starts)
        assert len(order) == len(set(order)) == min(64, Nk) and all(0 <= p < Nk for p in order)
        must = {0, 31, 32, 63, 64, Nk - 1} | {p for s in starts for p in (s - 1, s)}
        assert must <= set(order), (shape, sorted(must - set(order)))
        p = plans(*shape)
        n = len(order)
        for start in range(n):                                                # any rotation, any wave: 32 consecutive entries of the cycle
            wave = [order[(start + j) % n] for j in range(min(32, Nq))]
            assert len({k // 64 for k in wave}) >= min(2, T.cdiv(Nk, 64)), (shape, start)
            for kind in (T.FWD, T.DQ):
                groups = key_groups(Nk, p[kind]["ks"])
                assert {sum(k >= s for s in groups) for k in wave} == set(range(1, len(groups) + 1)), (shape, kind, start)
    for B, Nq, H, Nk in R.XATTN_CASES:
        order = R.designated_keys(Nk)
        assert len(order) == 64 and {0, 31, 32, 63, 64, Nk - 1} <= set(order)


# what the issue expects of the shapes, confirmed by the query: shape -> {kind: (ks, qw, db)} (+ dK/dV's query chunks)
EXPECTED = {
    (1, 2, 200, 77): {T.FWD: (1, 1, 0), T.DQ: (1, 1, 0)},
    (2, 3, 256, 256): {T.FWD: (2, 1, 1), T.DQ: (2, 1, 1)},
    (1, 2, 320, 1100): {T.FWD: (4, 2, 1), T.DQ: (4, 2, 1)},
    (9, 57, 64, 256): {T.DQ: (2, 4, 0)},
    (7, 37, 64, 256): {T.FWD: (2, 1, 0)},          # (two 32-row blocks per head: 2 x 37 x 7 = 518 workgroups, over the double buffer's 512)
}


def test_shapes_reach_every_launch_form():
    got = {s: plans(*s) for s in R.SHAPES}
    for s, p in got.items():
        assert math.prod(s) <= 1 << 24, s
        for kind in (T.FWD, T.DQ, T.DKV):
            T.check_derived((kind, *s, 0, T.DBG_SCRATCH if kind == T.DKV else 0), p[kind])
        print(s, {kind: tuple(p[kind][f] for f in T.PINNED) for kind in p})
    form = lambda p: (p["ks"], p["qw"], p["db"])
    for s, want in EXPECTED.items():
        for kind, f in want.items():
            assert form(got[s][kind]) == f, (s, kind, got[s][kind])
    assert got[(1, 2, 576, 77)][T.DKV]["qchunks"] == 4 and got[(1, 2, 576, 77)][T.DKV]["reduce"] == 1
    # 1100 keys, four groups of five tiles: the fourth group ends on a tile of 12 keys
    assert key_groups(1100, 4) == [0, 320, 640, 960] and 1100 - 17 * 64 == 12
    for kind in (T.FWD, T.DQ):
        ps = [(s, p[kind]) for s, p in got.items()]
        grid = lambda p: p["grid_x"] * p["grid_y"] * p["grid_z"]
        assert any(p["ks"] == 1 and T.cdiv(s[3], 64) >= 3 for s, p in ps), kind                # one group, at least three key tiles
        assert any(p["ks"] == 2 and p["db"] == 1 for s, p in ps), kind
        assert any(p["ks"] == 4 and p["db"] == 1 for s, p in ps), kind
        assert any(p["ks"] >= 2 and p["db"] == 0 and grid(p) > 512 for s, p in ps), kind        # key split, single buffer
        assert any(s[3] % 64 != 0 for s, p in ps) and any(s[3] % 64 == 0 for s, p in ps), kind  # ragged and whole last tiles
        assert any(p["ks"] > 1 and s[3] % 64 != 0 for s, p in ps), kind                         # ... also behind a key split
    dkv = [(s, p[T.DKV]) for s, p in got.items()]
    assert any(p["ks"] == 1 and not p["reduce"] for s, p in dkv) and any(p["ks"] == 2 for s, p in dkv)
    assert any(p["reduce"] == 1 and p["qchunks"] > 1 and s[3] <= 128 for s, p in dkv)            # the few-key form
    for B, H, N in R.CAUSAL_SHAPES:
        p = T.named(T.plan(T.FWD, B, H, N, N, 1))
        assert p["launch"] == 1 and p["ks"] == 1
