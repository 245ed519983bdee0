"""Attention inputs over the logit range real checkpoints produce, with their float64 references: the helper of
tests/test_attention_range.py (CPU: a rounding model of the kernels, and which launches the shapes reach) and
tests/test_attention_range_gpu.py (the kernels).  Pure torch on the device it is given; nothing here calls the library.

Every family returns a dict with 16-bit q [B][Nq][H 64], k, v [B][Nk][H 64], do [B][Nq][H 64] and `ref`, the float64 attention of
exactly those rounded tensors (head width 64, scale 0.125): o, lse, dq, dk, dv.

  scaled(sigma)  unit-normal q, k, v, dO; q times sigma.  sigma = 16: logits of standard deviation 16, the largest of a 320 x 1100 head about 78.
  shifted(c = 4) unit-normal draws, then q + 2 and k + c: every logit of a row moves by a common amount of several tens of nats,
                 so |m| and |lse| are large at unit spread.  (c stays 4: at c = 16 the 16-bit rounding of dS alone takes dq past
                 its tolerance, because k then has a large common component; that is no property of a kernel.)
  sink(L = 10)   q = 1; k = 0 except one key per head whose entries are L / 8: that key has logit L, every other key logit 0.
                 v = 1 on the flat keys, random on the sink key; dO random.  Meant for Nk >= 1024: a thousand flat keys 10 nats
                 under the sink hold 4.7 % of the row's mass in probabilities that are subnormal in fp16.
  uniform        q = 0: o = mean(v), lse = ln Nk.
  one_hot        exact.  Codes = the 64 rows of the 64 x 64 Hadamard matrix times 3: two distinct codes have logit 0, equal codes
                 logit 72, exactly, in both 16-bit types.  At most 64 designated keys carry one code each, every other key is 0;
                 query i carries the code of its designated key.  v and dO hold integers in [-2, 2], so every f32 dot product is
                 exact in any summation order.  The causal form (N > 64): k_j = code(j mod 64), q_i = code(i mod 64), so row i
                 attends equally to the keys j = i (mod 64), j <= i, and the newest visible key is always a winner."""
import math

import torch

HD = 64
SCALE = 0.125
ONE_HOT_LOGIT = 72.0           # 3 * 3 * 64 / 8

# (B, H, Nq, Nk) of the flash-kernel cases; tests/test_attention_range.py asserts which launches they reach.  B H Nq Nk <= 2^24, so
# that a case and its float64 reference take a few seconds at most.  (The 16-wave forward, ks = 4 with four row waves, needs at
# least 4033 keys on a full grid: it stays with the unit-variance shapes of tests/test_unet_kernels_gpu.py.)
SHAPES = [(1, 2, 200, 77), (1, 2, 100, 192), (2, 3, 256, 256), (1, 2, 320, 1100), (1, 2, 576, 77), (9, 57, 64, 256),
          (7, 37, 64, 256)]
CAUSAL_SHAPES = [(1, 16, 77), (1, 2, 65), (1, 3, 129)]                                     # (B, H, N)
XATTN_CASES = [(1, 64, 1, 77), (1, 200, 2, 77), (2, 128, 2, 77), (1, 64, 1, 96)]           # (B, Nq, H, Nk)
SINK_MIN_KEYS = 1024


def flash_families(Nk):
    """the random families a flash-kernel shape runs (one_hot is on every shape as well)"""
    return ["scaled4", "scaled16", "shifted", "uniform"] + (["sink"] if Nk >= SINK_MIN_KEYS else [])


def heads(t, H):
    """[B][N][H 64] -> [B][H][N][64]"""
    B, N, _ = t.shape
    return t.reshape(B, N, H, HD).transpose(1, 2)


def unheads(t):
    """[B][H][N][64] -> [B][N][H 64]"""
    B, H, N, _ = t.shape
    return t.transpose(1, 2).reshape(B, N, H * HD)


def logits(q, k, H, causal=False):
    """float64 logits [B][H][Nq][Nk]; causal: key j hidden from query i for j > i"""
    s = (heads(q.double(), H) @ heads(k.double(), H).transpose(-1, -2)) * SCALE
    if causal:
        Nq, Nk = s.shape[-2:]
        s = s.masked_fill(torch.ones(Nq, Nk, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    return s


def reference(q, k, v, do, H, causal=False):
    """float64 attention forward and backward of the given (16-bit) tensors, in closed form"""
    Q, K, V, DO = (heads(t.double(), H) for t in (q, k, v, do))
    s = logits(q, k, H, causal)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    del s
    o = p @ V
    dv = p.transpose(-1, -2) @ DO
    ds = p * (DO @ V.transpose(-1, -2) - (DO * o).sum(-1, keepdim=True))
    del p
    dq = (ds @ K) * SCALE
    dk = (ds.transpose(-1, -2) @ Q) * SCALE
    return dict(o=unheads(o), lse=lse, dq=unheads(dq), dk=unheads(dk), dv=unheads(dv))


def model(q, k, v, do, H, dtype, flush_subnormal=False):
    """The kernels' roundings in float64 arithmetic: the unnormalised P = exp(s - max) is rounded to the 16-bit type before P V
    (the row sum keeps the unrounded values), o is rounded, delta = rowsum(dO o) takes that rounded o, lse is stored in f32, the
    backward's P = exp(s - lse) and dS = P (dP - delta) are rounded before their products, and the outputs are rounded.
    flush_subnormal: probabilities below the smallest normal number of the type become zero (what a kernel that flushed fp16
    subnormals would compute; the kernels do not)."""
    rnd = lambda t: t.to(dtype).double()
    tiny = torch.finfo(dtype).tiny
    prob = (lambda t: torch.where(rnd(t) < tiny, torch.zeros_like(t), rnd(t))) if flush_subnormal else rnd
    Q, K, V, DO = (heads(t.double(), H) for t in (q, k, v, do))
    s = logits(q, k, H)
    m = s.amax(dim=-1, keepdim=True)
    pu = torch.exp(s - m)
    l = pu.sum(-1, keepdim=True)
    o = rnd((prob(pu) @ V) / l)
    lse = (m + torch.log(l)).float().double()
    del pu
    p = torch.exp(s - lse)
    del s
    ds = rnd(p * (DO @ V.transpose(-1, -2) - (DO * o).sum(-1, keepdim=True)))
    dv = rnd(prob(p).transpose(-1, -2) @ DO)
    del p
    dq = rnd((ds @ K) * SCALE)
    dk = rnd((ds.transpose(-1, -2) @ Q) * SCALE)
    return dict(o=unheads(o), lse=lse[..., 0], dq=unheads(dq), dk=unheads(dk), dv=unheads(dv))


def _gen(seed):
    """Every draw comes from the CPU generator and is then moved: a case holds the same numbers on every device, so what the
    CPU test's rounding model says of a case it says of the tensors the kernels get."""
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _randn(shape, g, device):
    return torch.randn(*shape, generator=g).to(device)


def _case(q, k, v, do, H, dtype, causal=False, **extra):
    q, k, v, do = (t.to(dtype).contiguous() for t in (q, k, v, do))
    return dict(q=q, k=k, v=v, do=do, H=H, dtype=dtype, ref=reference(q, k, v, do, H, causal), **extra)


def scaled(sigma, dtype, B, H, Nq, Nk, device, seed=0, causal=False):
    g = _gen(seed)
    C = H * HD
    q, do = (_randn((B, Nq, C), g, device) for _ in range(2))
    k, v = (_randn((B, Nk, C), g, device) for _ in range(2))
    return _case(q * sigma, k, v, do, H, dtype, causal)


def shifted(dtype, B, H, Nq, Nk, device, seed=0, c=4.0):
    g = _gen(seed)
    C = H * HD
    q, do = (_randn((B, Nq, C), g, device) for _ in range(2))
    k, v = (_randn((B, Nk, C), g, device) for _ in range(2))
    return _case(q + 2.0, k + c, v, do, H, dtype)


def sink_key(b, h, Nk):
    """the sink key of head h of image b: another tile and another place inside the tile for every head"""
    return (Nk // 3 + 67 * h + 13 * b) % Nk


def sink(dtype, B, H, Nq, Nk, device, seed=0, L=10.0):
    g = _gen(seed)
    C = H * HD
    q = torch.ones(B, Nq, C, device=device)
    do = _randn((B, Nq, C), g, device)
    k = torch.zeros(B, Nk, H, HD, device=device)
    v = torch.ones(B, Nk, H, HD, device=device)
    vs = _randn((B, H, HD), g, device)
    for b in range(B):
        for h in range(H):
            k[b, sink_key(b, h, Nk), h] = L / 8.0
            v[b, sink_key(b, h, Nk), h] = vs[b, h]
    return _case(q, k.reshape(B, Nk, C), v.reshape(B, Nk, C), do, H, dtype)


def uniform(dtype, B, H, Nq, Nk, device, seed=0):
    g = _gen(seed)
    C = H * HD
    do = _randn((B, Nq, C), g, device)
    k, v = (_randn((B, Nk, C), g, device) for _ in range(2))
    return _case(torch.zeros(B, Nq, C, device=device), k, v, do, H, dtype)


def codes(device):
    """the 64 rows of the Sylvester Hadamard matrix of order 64, times 3"""
    h = torch.ones(1, 1, device=device)
    for _ in range(6):
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return 3.0 * h


def designated_keys(Nk, group_starts=()):
    """At most 64 key positions that carry a code: keys 0, 31, 32, 63, 64 and Nk - 1, both sides of every tile boundary a key
    group starts on (group_starts: first key of each group after the first), and a scattering of the rest.  They come back in the
    order the queries cycle through them: the keys of every 64-key tile spread evenly over the cycle, so that 32 consecutive
    rows (one wave) have winners in as many tiles, and key groups, as the cycle has."""
    want = [0, 31, 32, 63, 64, Nk - 1]
    for s in group_starts:
        want += [s - 1, s]
    keys = []
    for p in want:
        if 0 <= p < Nk and p not in keys:
            keys.append(p)
    assert len(keys) <= 64
    i = 0
    while len(keys) < min(64, Nk):
        p = (17 + 97 * i) % Nk
        i += 1
        if p not in keys:
            keys.append(p)
    tiles = {}
    for p in sorted(keys):
        tiles.setdefault(p // 64, []).append(p)
    rank = {p: ((a + 0.5) / len(ps), t) for t, ps in tiles.items() for a, p in enumerate(ps)}
    return sorted(keys, key=rank.get)


def _integers(shape, g, device):
    return torch.randint(-2, 3, shape, generator=g).float().to(device)


def one_hot(dtype, B, H, Nq, Nk, device, seed=0, group_starts=()):
    """`winner` [B][H][Nq]: the one key of logit 72 of every row (all other logits are 0)"""
    g = _gen(seed)
    C = H * HD
    order = torch.tensor(designated_keys(Nk, group_starts), device=device)
    nd, code = len(order), codes(device)
    k = torch.zeros(B, Nk, H, HD, device=device)
    q = torch.zeros(B, Nq, H, HD, device=device)
    winner = torch.zeros(B, H, Nq, dtype=torch.long, device=device)
    rows = torch.arange(Nq, device=device)
    for b in range(B):
        for h in range(H):
            idx = (rows + 5 * h + 3 * b) % nd          # another rotation of the cycle for every head
            k[b, order, h] = code[:nd]
            q[b, :, h] = code[idx]
            winner[b, h] = order[idx]
    return _case(q.reshape(B, Nq, C), k.reshape(B, Nk, C), _integers((B, Nk, C), g, device), _integers((B, Nq, C), g, device), H,
                 dtype, winner=winner, designated=order)


def one_hot_causal(dtype, B, H, N, device, seed=0):
    g = _gen(seed)
    C = H * HD
    rows = codes(device)[torch.arange(N, device=device) % 64]                   # [N][64]
    qk = rows[None, :, None, :].expand(B, N, H, HD).reshape(B, N, C)
    return _case(qk, qk, _integers((B, N, C), g, device), _integers((B, N, C), g, device), H, dtype, causal=True)


def winners(c, causal=False):
    """[B][H][Nq][Nk] bool: the keys of a one_hot case whose logit is 72 (exact in float64)"""
    return logits(c["q"], c["k"], c["H"], causal) == ONE_HOT_LOGIT


# The sink key's dk is ONE number per head, repeated over the 64 columns (q = 1 in every row): the sum over all Nq rows of
# dS[i][sink] = p (dP_i - delta_i), whose error is the sum of the rows' delta errors -- delta_i = rowsum(dO_i o_i) takes the 16-bit
# o, and v = 1 on the flat keys gives o a common component that this rounding turns into an error of delta (the amplification
# every flash attention has for a v with a common offset).  Against a true dk[sink] that is itself a sum of Nq terms of random
# sign, the rounding model's ratio of that one number ranges over the draws from 0.06 to 3.2 of tolerance in bf16 (twelve seeds at
# (1, 2, 320, 1100): four over 1, 0.84 at most in fp16), every other element staying below 0.7.  The sink case therefore runs on
# a fixed draw on which the MODEL stays below 0.8 in both types (tests/test_attention_range.py asserts it); the draws are the
# same on every device, so the kernels get the tensors the model passed.
SINK_SEED = 0


def seed_of(family, B, H, Nq, Nk):
    return SINK_SEED if family == "sink" else B + H + Nq + Nk


def make(family, dtype, B, H, Nq, Nk, device, seed=None, group_starts=()):
    seed = seed_of(family, B, H, Nq, Nk) if seed is None else seed
    if family == "scaled4":
        return scaled(4.0, dtype, B, H, Nq, Nk, device, seed)
    if family == "scaled16":
        return scaled(16.0, dtype, B, H, Nq, Nk, device, seed)
    if family == "shifted":
        return shifted(dtype, B, H, Nq, Nk, device, seed)
    if family == "sink":
        assert Nk >= SINK_MIN_KEYS
        return sink(dtype, B, H, Nq, Nk, device, seed)
    if family == "uniform":
        return uniform(dtype, B, H, Nq, Nk, device, seed)
    if family == "one_hot":
        return one_hot(dtype, B, H, Nq, Nk, device, seed, group_starts)
    raise ValueError(family)


def uniform_lse(Nk):
    return math.log(Nk)
