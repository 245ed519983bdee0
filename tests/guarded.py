"""Guard bands around device buffers, for the tests of everything that takes caller memory (tests/test_workspace_guards_gpu.py).

torch's caching allocator rounds every request to 512 bytes and hands out pieces of large blocks, so a kernel that writes past
the end of a tensor lands in slack or in a neighbour and no test sees it.  A `Frame` hands out tensors that are views into a
uint8 buffer of its own with GUARD bytes on each side: the data starts 256-aligned (what the kernels may assume of a torch
allocation), the rear guard starts at the first byte behind the data, with no rounding.  `TorchProxy` stands in for the `torch`
name of ONE product module (monkeypatch.setattr(module, "torch", proxy)): the device allocations that module makes -- where the
sizes of the outputs and workspaces are decided -- then come from the frame, and everything else is torch's.

A frame also keeps the bytes every buffer held when it was handed out, so a test can say "this part is what it was before the
call" of any piece of a frame tensor: a guard (`check`), the gaps between the sub-buffers of a workspace arena
(`check_arena_gaps`, with the take log of dh_dbg_arena_log), or the elements an interface documents as unwritten (`unchanged`,
`tail_unchanged`)."""
import ctypes
import sys

import torch

GUARD = 4096
FILLS = ("zeros", "ones", "random")          # 0x00, 0xFF, seeded random bytes


class _Rec:
    __slots__ = ("name", "buf", "start", "nbytes", "before", "addr", "tensor")


class Frame:
    def __init__(self, fill, device, seed=1234):
        assert fill in FILLS, fill
        self.fill, self.device = fill, torch.device(device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)
        self.recs = []

    # ---- handing out ---------------------------------------------------------------------------------------------------------
    def _random(self, n):
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device=self.device, generator=self.gen)

    def alloc(self, shape, dtype, name, value=None):
        """A contiguous tensor of `shape` / `dtype` inside guards.  value None: the frame's fill (what torch.empty stands for);
        else every element is `value`.  The guards always hold random bytes, so no constant a stray memset writes hides in them."""
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        item = torch.empty(0, dtype=dtype).element_size()
        nbytes = numel * item
        buf = torch.empty(GUARD + 255 + nbytes + GUARD, dtype=torch.uint8, device=self.device)
        start = GUARD + (-(buf.data_ptr() + GUARD)) % 256
        buf[:start] = self._random(start)
        buf[start + nbytes:] = self._random(buf.numel() - start - nbytes)
        data = buf[start:start + nbytes]
        t = data.view(dtype).view(shape)
        if value is not None:
            t.fill_(value)
        elif self.fill == "random":
            data.copy_(self._random(nbytes))
        else:
            data.fill_(0 if self.fill == "zeros" else 255)
        r = _Rec()
        r.name, r.buf, r.start, r.nbytes, r.addr = f"{name} {list(shape)} {str(dtype).replace('torch.', '')}", buf, start, nbytes, buf.data_ptr() + start
        assert r.addr % 256 == 0 and (nbytes == 0 or r.addr == t.data_ptr())
        r.before, r.tensor = buf.clone(), t
        self.recs.append(r)
        return t

    # ---- looking up ----------------------------------------------------------------------------------------------------------
    def rec_of(self, addr):
        """The record whose data holds the address (its end included: an empty slice at the end of a tensor), or None."""
        for r in self.recs:
            if r.addr <= addr <= r.addr + r.nbytes:
                return r
        return None

    def find(self, shape, dtype):
        """The tensors handed out with this shape and dtype, in order (an output the caller does not return)."""
        return [r.tensor for r in self.recs if tuple(r.tensor.shape) == tuple(shape) and r.tensor.dtype == dtype]

    def _span(self, t):
        assert t.is_contiguous(), "contiguous pieces only"
        r = self.rec_of(t.data_ptr())
        assert r is not None, "not a piece of a frame tensor"
        off = r.start + t.data_ptr() - r.addr
        n = t.numel() * t.element_size()
        assert off + n <= r.start + r.nbytes, "the piece leaves its tensor"
        return r, off, n

    @staticmethod
    def _first_diff(a, b):
        d = (a != b).nonzero()
        return None if d.numel() == 0 else int(d[0, 0])

    # ---- checks --------------------------------------------------------------------------------------------------------------
    def check(self):
        """(a) every guard byte of every tensor handed out is what it was."""
        for r in self.recs:
            for side, lo, hi in (("front", 0, r.start), ("rear", r.start + r.nbytes, r.buf.numel())):
                at = self._first_diff(r.buf[lo:hi], r.before[lo:hi])
                if at is not None:
                    where = f"{r.start - at} before the data" if side == "front" else f"{at} past the end of the data"
                    raise AssertionError(f"{r.name}: {side} guard changed, first at byte {where} (fill {self.fill})")

    def unchanged(self, t, what):
        """(c) the contiguous piece `t` of a frame tensor holds the bytes it was handed out with."""
        if t.numel() == 0:
            return
        r, off, n = self._span(t)
        at = self._first_diff(r.buf[off:off + n], r.before[off:off + n])
        assert at is None, f"{what}: {r.name} changed where the interface leaves it alone, first at byte {off - r.start + at} (fill {self.fill})"

    def tail_unchanged(self, t, what):
        """(c) everything of t's frame tensor that lies behind the contiguous piece `t` (a list's tail behind its count)."""
        r, off, n = self._span(t)
        lo, hi = off + n, r.start + r.nbytes
        at = self._first_diff(r.buf[lo:hi], r.before[lo:hi])
        assert at is None, f"{what}: {r.name} changed behind its written part, first at byte {lo - r.start + at} (fill {self.fill})"

    def check_arena_gaps(self, takes):
        """(b) `takes`: the rows (base address, offset, bytes) of dh_dbg_arena_log_read.  For every arena whose base lies in a frame
        tensor: every byte from the base to the end of that tensor that no take of the arena covers -- the alignment padding, the
        gap behind every take, the slack behind the last -- is what it was before the call.  Returns how many arenas it judged."""
        arenas, open_ = [], {}          # an arena: the takes of one base with ascending offsets (other arenas may carve in between)
        for base, off, nbytes in takes:
            parts = open_.get(base)
            if parts is None or off < parts[-1][0] + parts[-1][1]:
                parts = open_[base] = []
                arenas.append((base, parts))
            parts.append((off, nbytes))
        judged = 0
        for base, parts in arenas:
            if base == 0:
                continue
            r = self.rec_of(base)
            if r is None:
                continue
            judged += 1
            lo = r.start + base - r.addr
            span = r.start + r.nbytes - lo
            free = torch.ones(span, dtype=torch.bool, device=self.device)
            for off, nbytes in parts:
                assert off + nbytes <= span, f"{r.name}: a take [{off}, {off + nbytes}) of its arena leaves the tensor ({span} bytes)"
                free[off:off + nbytes] = False
            changed = (r.buf[lo:lo + span] != r.before[lo:lo + span]) & free
            at = self._first_diff(changed, torch.zeros_like(changed))
            if at is not None:
                k = max(i for i, (off, _) in enumerate(parts) if off <= at)
                off, nbytes = parts[k]
                raise AssertionError(f"{r.name}: arena byte {at} changed, {at - off - nbytes} bytes past the end of take {k} of "
                                     f"{len(parts)} ([{off}, {off + nbytes})) (fill {self.fill})")
        return judged


class TorchProxy:
    """`torch` for one module: empty / zeros / full and their _like forms on the frame's device come from the frame."""

    def __init__(self, frame):
        self._frame = frame

    def __getattr__(self, name):
        return getattr(torch, name)

    def _mine(self, device):
        if device is None:
            return False
        d = torch.device(device)
        return d.type == self._frame.device.type and (d.index is None or d.index == self._frame.device.index)

    @staticmethod
    def _where(fn):
        """fn@file:line of the product line that allocates (the first frame outside this file)"""
        f = sys._getframe(1)
        while f.f_code.co_filename == __file__:
            f = f.f_back
        return f"{fn}@{f.f_code.co_filename.rsplit('/', 1)[-1]}:{f.f_lineno}"

    @staticmethod
    def _shape(size):
        return tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)

    def _make(self, fn, size, value, dtype, device, kw):
        if not self._mine(device) or kw:
            return None
        return self._frame.alloc(self._shape(size), dtype or torch.get_default_dtype(), self._where(fn), value)

    def empty(self, *size, dtype=None, device=None, **kw):
        t = self._make("empty", size, None, dtype, device, kw)
        return torch.empty(*size, dtype=dtype, device=device, **kw) if t is None else t

    def zeros(self, *size, dtype=None, device=None, **kw):
        t = self._make("zeros", size, 0, dtype, device, kw)
        return torch.zeros(*size, dtype=dtype, device=device, **kw) if t is None else t

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if dtype is None or not self._mine(device) or kw:
            return torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        return self._frame.alloc(self._shape((size,)), dtype, self._where("full"), fill_value)

    def _like(self, fn, t, value, dtype, device, kw, fallback):
        if not self._mine(t.device if device is None else device) or kw:
            return fallback()
        return self._frame.alloc(tuple(t.shape), dtype or t.dtype, self._where(fn), value)

    def empty_like(self, t, dtype=None, device=None, **kw):
        return self._like("empty_like", t, None, dtype, device, kw, lambda: torch.empty_like(t, dtype=dtype, device=device, **kw))

    def zeros_like(self, t, dtype=None, device=None, **kw):
        return self._like("zeros_like", t, 0, dtype, device, kw, lambda: torch.zeros_like(t, dtype=dtype, device=device, **kw))

    def full_like(self, t, fill_value, dtype=None, device=None, **kw):
        return self._like("full_like", t, fill_value, dtype, device, kw,
                          lambda: torch.full_like(t, fill_value, dtype=dtype, device=device, **kw))


# ---- the arena hooks (csrc/debug_api.cpp) -----------------------------------------------------------------------------------------
def arena_gap(L, nbytes):
    return L.dh_dbg_arena_gap(int(nbytes))


def arena_log_start(L):
    assert L.dh_dbg_arena_log(1) == 0


def arena_log_read(L):
    """The takes recorded since the log was enabled: a list of (base address, offset, bytes)."""
    n = ctypes.c_int(0)
    assert L.dh_dbg_arena_log_read(None, 0, ctypes.byref(n)) == 0
    out = (ctypes.c_int64 * (3 * max(n.value, 1)))()
    assert L.dh_dbg_arena_log_read(out, n.value, ctypes.byref(n)) == 0
    return [(int(out[3 * i]), int(out[3 * i + 1]), int(out[3 * i + 2])) for i in range(n.value)]


def arena_reset(L):
    L.dh_dbg_arena_log(0)
    L.dh_dbg_arena_gap(0)
