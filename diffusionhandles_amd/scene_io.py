"""Scene-directory I/O for the edit harness (SURVEY section 8c "what the build's own counterparts must reproduce").

The reference's harness (`test/test_diffusion_handles.py:208-263`, `test/utils.py:8-58`) reads a scene directory
`input.png, mask.png, depth.exr, bg_depth.exr, prompt.txt, transforms.json` through imageio/torchvision, neither of
which is installed here.  This module reads the same files with the standard library + NumPy only:

* `read_png`   8/16-bit gray, gray+alpha, RGB, RGBA and palette PNGs, non-interlaced (all five scanline filters)
* `read_exr`   single-part scanline OpenEXR, HALF/FLOAT/UINT channels, compression NONE / ZIPS / ZIP / PIZ
               (the reference's depth maps are one HALF channel `Y`, PIZ-compressed, `lineOrder` decreasing)
* `write_png`  8-bit gray / RGB
* `load_scene` the reference loader's steps: centre crop, antialiased bilinear resize, mask > 0.5, first prompt line,
               ordered transforms `{name: {translation, rotation_axis, rotation_angle}}`

Host-side plumbing only: nothing here is on the timed path.
"""
import json
import os
import struct
import zlib
from collections import OrderedDict

import numpy as np

# ---------------------------------------------------------------------------------------------- PNG

_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def _paeth_row(cur, prev, bpp):
    out = bytearray(cur)
    for i in range(len(out)):
        a = out[i - bpp] if i >= bpp else 0
        b = prev[i]
        c = prev[i - bpp] if i >= bpp else 0
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
        out[i] = (out[i] + pred) & 255
    return out


def _avg_row(cur, prev, bpp):
    out = bytearray(cur)
    for i in range(len(out)):
        a = out[i - bpp] if i >= bpp else 0
        out[i] = (out[i] + ((a + prev[i]) >> 1)) & 255
    return out


def _sub_row(cur, bpp):
    a = np.frombuffer(bytes(cur), dtype=np.uint8).reshape(-1, bpp).astype(np.uint32)
    return bytearray((np.cumsum(a, axis=0) & 255).astype(np.uint8).tobytes())


def read_png(path):
    """-> uint8 or uint16 array [H,W] (gray) or [H,W,C]."""
    with open(path, "rb") as f:
        b = f.read()
    if b[:8] != _PNG_SIG:
        raise ValueError(f"{path}: not a PNG file")
    p, idat, hdr, plte = 8, [], None, None
    while p < len(b):
        n, tag = struct.unpack(">I4s", b[p:p + 8])
        data = b[p + 8:p + 8 + n]
        p += 12 + n
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", data)
        elif tag == b"IDAT":
            idat.append(data)
        elif tag == b"PLTE":
            plte = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3)
        elif tag == b"IEND":
            break
    if hdr is None:
        raise ValueError(f"{path}: no IHDR chunk")
    w, h, depth, ctype, _, _, interlace = hdr
    if interlace:
        raise ValueError(f"{path}: interlaced PNGs are not supported")
    nch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    bits = nch * depth
    bpp = max(1, bits // 8)
    stride = (w * bits + 7) // 8
    raw = zlib.decompress(b"".join(idat))
    if len(raw) < h * (stride + 1):
        raise ValueError(f"{path}: truncated image data")
    rows, prev = [], bytearray(stride)
    for y in range(h):
        ft = raw[y * (stride + 1)]
        cur = raw[y * (stride + 1) + 1:(y + 1) * (stride + 1)]
        if ft == 0:
            cur = bytearray(cur)
        elif ft == 1:
            cur = _sub_row(cur, bpp)
        elif ft == 2:
            cur = bytearray(((np.frombuffer(cur, dtype=np.uint8).astype(np.uint16) + np.frombuffer(bytes(prev), dtype=np.uint8)) & 255)
                            .astype(np.uint8).tobytes())
        elif ft == 3:
            cur = _avg_row(cur, prev, bpp)
        elif ft == 4:
            cur = _paeth_row(cur, prev, bpp)
        else:
            raise ValueError(f"{path}: bad filter type {ft}")
        rows.append(bytes(cur))
        prev = cur
    data = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(h, stride)
    if depth == 16:
        img = data.view(">u2").astype(np.uint16).reshape(h, w, nch)
    elif depth == 8:
        img = data.reshape(h, w, nch)
    else:                                           # 1/2/4-bit gray or palette: unpack MSB first
        per = 8 // depth
        shifts = np.arange(per - 1, -1, -1, dtype=np.uint8) * depth
        img = ((data[:, :, None] >> shifts[None, None, :]) & ((1 << depth) - 1)).reshape(h, stride * per)[:, :w, None]
        if ctype == 0:
            img = (img.astype(np.uint16) * (255 // ((1 << depth) - 1))).astype(np.uint8)
    if ctype == 3:
        if plte is None:
            raise ValueError(f"{path}: palette image without PLTE")
        img = plte[img[..., 0]]
    return img[..., 0] if img.shape[-1] == 1 else img


def write_png(path, img):
    """img: [H,W] or [H,W,3] float in [0,1] (or uint8).  `save_image` of test/utils.py:21-31 truncates (`* 255` ->
    uint8), so does this."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        a = (np.clip(a, 0, 1) * 255.0).astype(np.uint8)
    if a.ndim == 2:
        a = a[..., None]
    h, w, c = a.shape
    raw = b"".join(b"\x00" + a[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    hdr = struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[c], 0, 0, 0)
    with open(path, "wb") as f:
        f.write(_PNG_SIG + chunk(b"IHDR", hdr) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


# ---------------------------------------------------------------------------------------------- OpenEXR

_EXR_MAGIC = 20000630
_LINES = {0: 1, 1: 1, 2: 1, 3: 16, 4: 32}          # NONE, RLE, ZIPS, ZIP, PIZ
_PIX_BYTES = {0: 4, 1: 2, 2: 4}                    # UINT, HALF, FLOAT
_PIX_DTYPE = {0: "<u4", 1: "<f2", 2: "<f4"}


def _cstr(b, p):
    e = b.index(b"\0", p)
    return b[p:e].decode("latin-1"), e + 1


def _exr_header(b):
    magic, version = struct.unpack("<II", b[:8])
    if magic != _EXR_MAGIC:
        raise ValueError("not an OpenEXR file")
    if version & 0x200 or version & 0x1000 or version & 0x800:
        raise ValueError("tiled / multi-part / deep OpenEXR files are not supported")
    p, attrs = 8, {}
    while b[p] != 0:
        name, p = _cstr(b, p)
        typ, p = _cstr(b, p)
        (sz,) = struct.unpack("<I", b[p:p + 4])
        attrs[name] = (typ, b[p + 4:p + 4 + sz])
        p += 4 + sz
    p += 1
    chans, v, q = [], attrs["channels"][1], 0
    while v[q] != 0:
        cn, q = _cstr(v, q)
        pt, _lin, xs, ys = struct.unpack("<IB3xii", v[q:q + 16])
        q += 16
        if xs != 1 or ys != 1:
            raise ValueError("sub-sampled OpenEXR channels are not supported")
        chans.append((cn, pt))
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    return dict(channels=chans, compression=attrs["compression"][1][0], window=(x0, y0, x1, y1)), p


def _zip_undo(data, expected):
    t = np.frombuffer(zlib.decompress(data), dtype=np.uint8).astype(np.int64)
    if t.size != expected:
        raise ValueError("OpenEXR zip block has the wrong size")
    t = (np.cumsum(t - 128) + 128) & 255 if t.size else t         # t[i] = t[i-1] + t[i] - 128
    t = t.astype(np.uint8)
    half = (t.size + 1) // 2
    out = np.empty(t.size, dtype=np.uint8)
    out[0::2] = t[:half]
    out[1::2] = t[half:]
    return out.tobytes()


# ---- PIZ: 16-bit value bitmap + LUT, Huffman-coded wavelet coefficients (OpenEXR's published format) ------

def _huf_unpack_table(b, p, im, iM):
    """6-bit code lengths im..iM, MSB-first, with zero-run codes 59..62 (2..5 zeros) and 63 (+8 bits: 6..261 zeros)."""
    lens = np.zeros(65537, dtype=np.int64)
    c = lc = 0

    def bits(n):
        nonlocal c, lc, p
        while lc < n:
            c = ((c << 8) | b[p]) & 0xFFFFFFFFFFFF
            p += 1
            lc += 8
        lc -= n
        return (c >> lc) & ((1 << n) - 1)

    i = im
    while i <= iM:
        l = bits(6)
        if l == 63:
            i += bits(8) + 6
        elif l >= 59:
            i += l - 59 + 2
        else:
            lens[i] = l
            i += 1
    return lens, p


def _huf_canonical(lens):
    """symbol -> code: codes of a length are consecutive in symbol order; the base of length l is
    (base(l+1) + count(l+1)) >> 1, from base(58) = 0."""
    n = np.bincount(lens, minlength=59).astype(object)
    base, c = [0] * 59, 0
    for l in range(58, 0, -1):
        nc = (c + int(n[l])) >> 1
        base[l] = c
        c = nc
    table = {}
    for s in np.nonzero(lens)[0]:
        l = int(lens[s])
        table[(1 << l) | base[l]] = int(s)            # leading one marks the length
        base[l] += 1
    return table


def _huf_uncompress(b, n_raw):
    im, iM, _tl, nbits, _r = struct.unpack("<5I", b[:20])
    if im > 65536 or iM > 65536:
        raise ValueError("bad PIZ Huffman header")
    lens, p = _huf_unpack_table(b, 20, im, iM)
    if nbits > 8 * (len(b) - p):
        raise ValueError("PIZ Huffman data is truncated")
    table, rlc = _huf_canonical(lens), iM
    out = np.empty(n_raw, dtype=np.uint16)
    get = table.get
    no = 0
    key = 1
    pos, end = p * 8, p * 8 + nbits
    while pos < end:
        key = (key << 1) | ((b[pos >> 3] >> (7 - (pos & 7))) & 1)
        pos += 1
        s = get(key)
        if s is None:
            if key >> 59:
                raise ValueError("bad PIZ Huffman code")
            continue
        key = 1
        if s == rlc:
            if pos + 8 > end or no == 0:
                raise ValueError("bad PIZ run")
            cs = 0
            for _ in range(8):
                cs = (cs << 1) | ((b[pos >> 3] >> (7 - (pos & 7))) & 1)
                pos += 1
            if no + cs > n_raw:
                raise ValueError("PIZ run overflows the block")
            out[no:no + cs] = out[no - 1]
            no += cs
        else:
            if no >= n_raw:
                raise ValueError("PIZ data overflows the block")
            out[no] = s
            no += 1
    if no != n_raw:
        raise ValueError(f"PIZ block decoded {no} of {n_raw} values")
    return out


def _wdec14(l, h):
    ls = l.astype(np.int16).astype(np.int32)
    hs = h.astype(np.int16).astype(np.int32)
    a = ls + (hs & 1) + (hs >> 1)
    return (a & 0xFFFF).astype(np.uint16), ((a - hs) & 0xFFFF).astype(np.uint16)


def _wdec16(l, h):
    m, d = l.astype(np.int32), h.astype(np.int32)
    bb = (m - (d >> 1)) & 0xFFFF
    aa = (d + bb - 0x8000) & 0xFFFF
    return aa.astype(np.uint16), bb.astype(np.uint16)


def _wav2_decode(a, mx):
    """In-place inverse 2-D wavelet of a [ny, nx] uint16 array (coarse to fine; whole levels at once)."""
    ny, nx = a.shape
    dec = _wdec14 if mx < (1 << 14) else _wdec16
    n = min(nx, ny)
    p = 1
    while p <= n:
        p <<= 1
    p >>= 1
    p2 = p
    p >>= 1
    while p >= 1:
        ys = np.arange(0, ny - p2 + 1, p2) if ny - p2 >= 0 else np.arange(0)
        xs = np.arange(0, nx - p2 + 1, p2) if nx - p2 >= 0 else np.arange(0)
        if len(ys) and len(xs):
            Y, X = np.ix_(ys, xs)
            px, p01, p10, p11 = a[Y, X], a[Y, X + p], a[Y + p, X], a[Y + p, X + p]
            i00, i10 = dec(px, p10)
            i01, i11 = dec(p01, p11)
            a[Y, X], a[Y, X + p] = dec(i00, i01)
            a[Y + p, X], a[Y + p, X + p] = dec(i10, i11)
        if nx & p and len(ys):                      # odd column left over at this level
            xo = len(xs) * p2
            i00, b10 = dec(a[ys, xo], a[ys + p, xo])
            a[ys, xo], a[ys + p, xo] = i00, b10
        if ny & p and len(xs):                      # odd row
            yo = len(ys) * p2
            i00, b01 = dec(a[yo, xs], a[yo, xs + p])
            a[yo, xs], a[yo, xs + p] = i00, b01
        p2 = p
        p >>= 1


def _piz_undo(data, chans, nx, ny):
    mn, mxnz = struct.unpack("<HH", data[:4])
    p = 4
    bitmap = np.zeros(8192, dtype=np.uint8)
    if mn <= mxnz:
        if mxnz >= 8192:
            raise ValueError("bad PIZ bitmap range")
        bitmap[mn:mxnz + 1] = np.frombuffer(data[p:p + mxnz - mn + 1], dtype=np.uint8)
        p += mxnz - mn + 1
    present = np.unpackbits(bitmap, bitorder="little").astype(bool)
    present[0] = True
    lut = np.zeros(65536, dtype=np.uint16)
    vals = np.nonzero(present)[0]
    lut[:len(vals)] = vals
    max_value = len(vals) - 1
    (length,) = struct.unpack("<i", data[p:p + 4])
    p += 4
    if length < 0 or p + length > len(data):
        raise ValueError("bad PIZ block length")
    sizes = [_PIX_BYTES[pt] // 2 for _, pt in chans]
    raw = _huf_uncompress(data[p:p + length], sum(nx * ny * s for s in sizes))
    planes, q = [], 0
    for s in sizes:
        blk = raw[q:q + nx * ny * s].reshape(ny, nx, s).copy()
        q += nx * ny * s
        for j in range(s):
            plane = np.ascontiguousarray(blk[:, :, j])
            _wav2_decode(plane, max_value)
            blk[:, :, j] = plane
        planes.append(lut[blk])
    # scan lines, channels in file order inside each line
    return b"".join(planes[c][y].astype("<u2").tobytes() for y in range(ny) for c in range(len(chans)))


def read_exr(path):
    """-> dict {channel name: float32 (or uint32) array [H,W]} of a single-part scanline file."""
    with open(path, "rb") as f:
        b = f.read()
    hdr, p = _exr_header(b)
    x0, y0, x1, y1 = hdr["window"]
    nx, ny = x1 - x0 + 1, y1 - y0 + 1
    comp, chans = hdr["compression"], hdr["channels"]
    if comp not in _LINES or comp == 1:
        raise ValueError(f"{path}: OpenEXR compression {comp} is not supported (NONE, ZIPS, ZIP, PIZ are)")
    lines = _LINES[comp]
    nchunks = (ny + lines - 1) // lines
    offsets = struct.unpack(f"<{nchunks}Q", b[p:p + 8 * nchunks])
    line_bytes = nx * sum(_PIX_BYTES[pt] for _, pt in chans)
    out = {cn: np.zeros((ny, nx), dtype=np.uint32 if pt == 0 else np.float32) for cn, pt in chans}
    for off in offsets:
        y, size = struct.unpack("<ii", b[off:off + 8])
        data = b[off + 8:off + 8 + size]
        rows = min(lines, y1 - y + 1)
        expected = rows * line_bytes
        if size < expected:
            if comp in (2, 3):
                data = _zip_undo(data, expected)
            elif comp == 4:
                data = _piz_undo(data, chans, nx, rows)
        elif size != expected:
            raise ValueError(f"{path}: bad chunk size")
        q = 0
        for r in range(rows):
            for cn, pt in chans:
                nb = nx * _PIX_BYTES[pt]
                out[cn][y - y0 + r] = np.frombuffer(data[q:q + nb], dtype=_PIX_DTYPE[pt])
                q += nb
    return out


def read_depth_exr(path):
    """`load_depth` (test/utils.py:33-42): the single channel of the file as float32 [H,W]."""
    ch = read_exr(path)
    for name in ("Y", "Z", "R", "depth"):
        if name in ch:
            return ch[name].astype(np.float32)
    return next(iter(ch.values())).astype(np.float32)


# ---------------------------------------------------------------------------------------------- scene directory

def crop_and_resize(img, size):
    """test/utils.py:54-58: centre crop to square, then bilinear resize with antialiasing (torchvision `resize`
    on a float tensor is `interpolate(mode='bilinear', align_corners=False, antialias=True)`).  img: torch [1,C,H,W]."""
    import torch.nn.functional as F
    h, w = img.shape[-2:]
    if h != w:
        s = min(h, w)
        top, left = int(round((h - s) / 2.0)), int(round((w - s) / 2.0))
        img = img[..., top:top + s, left:left + s]
    if img.shape[-1] != size:
        img = F.interpolate(img, size=(size, size), mode="bilinear", align_corners=False, antialias=True)
    return img


def load_image(path):
    """test/utils.py:8-19: float32 [C,H,W] in [0,1] (uint8 / 255)."""
    import torch
    a = read_png(path)
    if a.ndim == 2:
        a = a[..., None]
    scale = 255.0 if a.dtype == np.uint8 else 65535.0
    return torch.from_numpy(a.astype(np.float32) / scale).permute(2, 0, 1).contiguous()


MAX_SCENE_OBJECTS = 8          # losses.MAX_OBJECTS


def entry_instances(objects, n_masks=None, where="objects"):
    """The instance table of an "objects" list (copies of an object): None when no member carries "mask" (member n is then
    the object of mask n, as always), else one mask index per member -- its "mask": m, or its own position when it has none.
    ValueError naming `where` and the member for a "mask" that is not an integer >= 0 and, when n_masks is given, for more
    than 8 members, an index outside 0..n_masks-1 or a mask that no member draws."""
    if not any(isinstance(o, dict) and "mask" in o for o in objects):
        return None
    inst = []
    for n, o in enumerate(objects):
        m = o.get("mask", n) if isinstance(o, dict) else n
        if isinstance(m, bool) or not isinstance(m, int) or m < 0:
            raise ValueError(f"{where}, object {n}: \"mask\" must be the index of a mask (an integer >= 0), got {m!r}")
        inst.append(m)
    if n_masks is not None:
        if len(inst) > MAX_SCENE_OBJECTS:
            raise ValueError(f"{where} lists {len(inst)} instances, at most {MAX_SCENE_OBJECTS} are supported")
        for n, m in enumerate(inst):
            if m >= n_masks:
                raise ValueError(f"{where}, object {n}: mask {m} does not exist, the scene has {n_masks} object masks")
        for m in range(n_masks):
            if m not in inst:
                raise ValueError(f"{where}: no object draws mask {m} (removing an object is not supported)")
    return inst


def _is_donor(o):
    return isinstance(o, dict) and "donor" in o


def entry_donor(objects, n_donor=None, where="objects"):
    """Object insertion in an "objects" list (not in the reference): a member {"donor": d, ...transform keys} is an instance of
    mask d of the scene's donor image (donor/mask_d.png).  Returns None when no member carries "donor" (the list is then read as
    always), else (host members, donor members, the donor mask index of every donor member).  The donor members stand BEHIND the
    host's, as the donor's masks stand behind the host's in the edit's object list.  ValueError naming `where` and the member:
    a "donor" that is not an integer >= 0, a donor member that also carries "mask" or "remove", a host member behind a donor
    member, and, when n_donor is given, a scene without donor/ masks, an index outside 0..n_donor-1 or a donor mask that no
    member draws."""
    if not any(_is_donor(o) for o in objects):
        return None
    host, members, index = [], [], []
    for n, o in enumerate(objects):
        if not _is_donor(o):
            if members:
                raise ValueError(f"{where}, object {n}: a member of the host image stands behind a donor member (donor members "
                                 "come last)")
            host.append(o)
            continue
        d = o["donor"]
        if isinstance(d, bool) or not isinstance(d, int) or d < 0:
            raise ValueError(f"{where}, object {n}: \"donor\" must be the index of a donor mask (an integer >= 0), got {d!r}")
        for key in ("mask", "remove"):
            if key in o:
                raise ValueError(f"{where}, object {n}: a donor member takes no \"{key}\"")
        members.append(OrderedDict((k, v) for k, v in o.items() if k != "donor"))
        index.append(d)
    if n_donor is not None:
        if n_donor == 0:
            raise ValueError(f"{where}: a member carries \"donor\" but the scene has no donor/ directory with mask_0.png")
        if len(host) + len(members) > MAX_SCENE_OBJECTS:
            raise ValueError(f"{where} lists {len(host) + len(members)} instances, at most {MAX_SCENE_OBJECTS} are supported")
        for d in index:
            if d >= n_donor:
                raise ValueError(f"{where}: donor mask {d} does not exist, the scene's donor has {n_donor} masks")
        for d in range(n_donor):
            if d not in index:
                raise ValueError(f"{where}: no member draws donor mask {d} (an edit with a donor places every donor mask)")
    return host, members, index


def _is_removal(o):
    return isinstance(o, dict) and "remove" in o


def entry_removal(objects, n_masks=None, where="objects"):
    """Object removal in an "objects" list (not in the reference): a member {"remove": true} deletes the mask of its own position.
    Returns None when no member carries "remove" (the list is then read as always), else (removed, members, instances):
    the removed mask indices in order, the remaining members in order, and the mask index of every remaining member COUNTED
    AMONG THE REMAINING MASKS (its "mask", or its own position) -- None when that is 0, 1, 2 ... (no table needed).
    ValueError naming `where` and the member: "remove" that is not true, a removing member with any other key (a transform
    key, "mask"), a member that names a removed mask, and, when n_masks is given, a removing member beyond the masks, more than
    8 remaining members, a mask index outside the scene's or a remaining mask that no member draws."""
    if not any(_is_removal(o) for o in objects):
        return None
    removed, members, inst = [], [], []
    for n, o in enumerate(objects):
        if _is_removal(o):
            if o["remove"] is not True:
                raise ValueError(f"{where}, object {n}: \"remove\" must be true, got {o['remove']!r}")
            if len(o) != 1:
                other = sorted(k for k in o if k != "remove")
                raise ValueError(f"{where}, object {n}: a removed object takes no other key, got {other}")
            if n_masks is not None and n >= n_masks:
                raise ValueError(f"{where}, object {n}: \"remove\" deletes the mask of its own position, the scene has "
                                 f"{n_masks} object masks")
            removed.append(n)
    for n, o in enumerate(objects):
        if _is_removal(o):
            continue
        m = o.get("mask", n) if isinstance(o, dict) else n
        if isinstance(m, bool) or not isinstance(m, int) or m < 0:
            raise ValueError(f"{where}, object {n}: \"mask\" must be the index of a mask (an integer >= 0), got {m!r}")
        if m in removed:
            raise ValueError(f"{where}, object {n}: draws mask {m}, which object {m} removes")
        members.append(o)
        inst.append(m)
    if n_masks is not None:
        if len(inst) > MAX_SCENE_OBJECTS:
            raise ValueError(f"{where} lists {len(inst)} instances, at most {MAX_SCENE_OBJECTS} are supported")
        for o, m in zip(members, inst):
            if m >= n_masks:
                raise ValueError(f"{where}: mask {m} does not exist, the scene has {n_masks} object masks")
        for m in range(n_masks):
            if m not in inst and m not in removed:
                raise ValueError(f"{where}: no object draws mask {m} (an object is removed by {{\"remove\": true}} at its position)")
    inst = [m - sum(1 for r in removed if r < m) for m in inst]
    return removed, members, (None if inst == list(range(len(inst))) else inst)


def _check_object_entries(scene_dir, transforms, n_masks, n_donor=0):
    """transforms.json against the scene's masks: a multi-mask scene (n_masks >= 1 mask_m.png files) wants {"objects": [n_masks
    entries]} everywhere -- or, when members carry "mask" (copies of an object, entry_instances), n_masks to 8 entries that
    draw every mask -- a single-mask scene (n_masks = 0) no "objects" at all.  ValueError naming the scene and the entry."""
    for name, t in transforms.items():
        has = isinstance(t, dict) and "objects" in t
        if has and isinstance(t["objects"], (list, tuple)) and any(_is_donor(o) for o in t["objects"]):
            # donor members are checked by entry_donor; what is left is an ordinary entry of the host's members
            where = f"{scene_dir}: transform {name!r}"
            if n_masks == 0:
                raise ValueError(f"{where}: donor members need a multi-object scene (mask_0.png ...)")
            host, members, _ = entry_donor(t["objects"], n_donor, where)
            w = t.get("object_weights")
            rem = entry_removal(host, n_masks, where)
            n_left = len(host) - (0 if rem is None else len(rem[0]))
            if isinstance(w, (list, tuple)) and len(w) != n_left + len(members):
                raise ValueError(f"{where} has {len(w)} object_weights for {n_left + len(members)} instances")
            if n_masks + n_donor - (0 if rem is None else len(rem[0])) > MAX_SCENE_OBJECTS:
                raise ValueError(f"{where}: {n_masks} masks and {n_donor} donor masks, at most {MAX_SCENE_OBJECTS} in all")
            rest = OrderedDict((k, v) for k, v in t.items() if k != "object_weights")
            rest["objects"] = host
            _check_object_entries(scene_dir, {name: rest}, n_masks)
            continue
        if n_masks == 0 and _is_removal(t):          # a single-mask scene: {"remove": true} deletes the one object
            if t["remove"] is not True or len(t) != 1:
                raise ValueError(f"{scene_dir}: transform {name!r}: an entry that removes the object is exactly "
                                 f"{{\"remove\": true}}, got {dict(t)!r}")
            continue
        if n_masks > 0 and has and isinstance(t["objects"], (list, tuple)):
            rem = entry_removal(t["objects"], n_masks, f"{scene_dir}: transform {name!r}")
            if rem is not None:
                w = t.get("object_weights")
                if isinstance(w, (list, tuple)) and len(w) != len(rem[1]):
                    raise ValueError(f"{scene_dir}: transform {name!r} has {len(w)} object_weights for {len(rem[1])} remaining "
                                     "objects")
                if not rem[1] and w is not None:
                    raise ValueError(f"{scene_dir}: transform {name!r} removes every object and gives object_weights")
                continue
        if n_masks == 0:
            if has:
                raise ValueError(f"{scene_dir}: transform {name!r} has \"objects\" but the scene has one mask (mask.png, no mask_0.png)")
            continue
        if not has:
            raise ValueError(f"{scene_dir}: transform {name!r} has no \"objects\" list but the scene has {n_masks} object masks "
                             "(mask_0.png ...)")
        if isinstance(t["objects"], (list, tuple)) and \
                entry_instances(t["objects"], n_masks, f"{scene_dir}: transform {name!r}") is not None:
            w = t.get("object_weights")
            if isinstance(w, (list, tuple)) and len(w) != len(t["objects"]):
                raise ValueError(f"{scene_dir}: transform {name!r} has {len(w)} object_weights for {len(t['objects'])} instances")
            continue
        if not isinstance(t["objects"], (list, tuple)) or len(t["objects"]) != n_masks:
            n = len(t["objects"]) if isinstance(t["objects"], (list, tuple)) else "no"
            raise ValueError(f"{scene_dir}: transform {name!r} lists {n} objects, the scene has {n_masks} object masks")


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _check_similarity_entry(where, t):
    """The optional "scale" (a positive number or three) and "pivot" (three numbers) of one transforms.json entry; finite as
    float32, which is what the re-projection takes them as.  ValueError naming `where`."""
    if not isinstance(t, dict):
        return
    f32 = lambda v: float(np.float32(v))
    with np.errstate(over="ignore"):
        if "scale" in t:
            sc = t["scale"]
            vals = [sc] if _is_number(sc) else sc
            if not isinstance(vals, (list, tuple)) or len(vals) not in ((1,) if _is_number(sc) else (3,)) or \
                    not all(_is_number(v) for v in vals):
                raise ValueError(f"{where}: \"scale\" must be a number or a list of 3 numbers, got {sc!r}")
            if not all(np.isfinite(f32(v)) and f32(v) > 0.0 for v in vals):
                raise ValueError(f"{where}: \"scale\" must be positive and finite, got {sc!r}")
        if "pivot" in t:
            pv = t["pivot"]
            if not isinstance(pv, (list, tuple)) or len(pv) != 3 or not all(_is_number(v) for v in pv):
                raise ValueError(f"{where}: \"pivot\" must be a list of 3 numbers, got {pv!r}")
            if not all(np.isfinite(f32(v)) for v in pv):
                raise ValueError(f"{where}: \"pivot\" must be finite, got {pv!r}")


CAMERA_KEYS = ("rot_angle", "rot_axis", "translation", "pivot", "pivot_pixel")
BEND_KEYS = ("p0", "p1", "width", "bones", "pivot_pixel")
_TRANSFORM_KEYS = ("rotation_angle", "rotation_axis", "translation", "scale", "pivot", "objects", "remove", "object_weights", "bend")


def _check_bend_entry(where, t):
    """The optional "bend" of a member of "objects", or of the entry of a single-mask scene (not in the reference; bend edits): a
    dict {"p0": [x, y], "p1": [x, y] (pixels: the line the object bends across), "width" (pixels, > 0: the band that blends),
    "bones" (2 .. 4, default 2), "pivot_pixel" ([x, y], optional: the turn goes through the point of that pixel; default: the
    member's "pivot", else the midpoint of p0 p1)}.  The member's own rotation_angle / rotation_axis / translation are then
    the FULL motion of the far side, handed to depth_transform.bend_chain when the edit runs.  ValueError naming `where`."""
    if not isinstance(t, dict) or "bend" not in t:
        return
    b = t["bend"]
    if not isinstance(b, dict):
        raise ValueError(f"{where}: \"bend\" must be an object with {BEND_KEYS}, got {b!r}")
    extra = [k for k in b if k not in BEND_KEYS]
    if extra:
        raise ValueError(f"{where}: \"bend\" has unknown keys {extra} (known: {BEND_KEYS})")
    for key in ("p0", "p1", "width"):
        if key not in b:
            raise ValueError(f"{where}: \"bend\" needs \"{key}\"")
    for key in ("p0", "p1"):
        v = b[key]
        if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(_is_number(x) and np.isfinite(x) for x in v):
            raise ValueError(f"{where}: \"bend\": \"{key}\" must be a pixel [x, y], two finite numbers, got {v!r}")
    if [float(x) for x in b["p0"]] == [float(x) for x in b["p1"]]:
        raise ValueError(f"{where}: \"bend\": \"p0\" and \"p1\" are one pixel ({b['p0']!r}): no line")
    if not (_is_number(b["width"]) and np.isfinite(b["width"]) and b["width"] > 0):
        raise ValueError(f"{where}: \"bend\": \"width\" must be a positive number of pixels, got {b['width']!r}")
    n = b.get("bones", 2)
    if not (isinstance(n, int) and not isinstance(n, bool) and 2 <= n <= 4):
        raise ValueError(f"{where}: \"bend\": \"bones\" must be 2, 3 or 4, got {n!r}")
    if "pivot_pixel" in b:
        v = b["pivot_pixel"]
        if "pivot" in t:
            raise ValueError(f"{where}: \"bend\" has \"pivot_pixel\" and the entry a \"pivot\"")
        if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(isinstance(x, int) and not isinstance(x, bool) and x >= 0 for x in v):
            raise ValueError(f"{where}: \"bend\": \"pivot_pixel\" must be [x, y], two integers >= 0, got {v!r}")
    if "scale" in t:
        raise ValueError(f"{where}: an entry with \"bend\" takes no \"scale\" (the bones of a bend chain are rigid)")
    if "remove" in t or "objects" in t:
        raise ValueError(f"{where}: \"bend\" belongs to one object: a member of \"objects\", or the entry of a single-mask scene")


def bend_args(t):
    """The "bend" of one entry -> None (no key), or dict(p0, p1, width, bones) with `pivot_pixel` ((x, y)) when it gives one: the
    keyword arguments of depth_transform.bend_chain that do not come from the entry's own transform keys."""
    if not isinstance(t, dict) or "bend" not in t:
        return None
    _check_bend_entry("bend_args", t)
    b = t["bend"]
    out = dict(p0=(float(b["p0"][0]), float(b["p0"][1])), p1=(float(b["p1"][0]), float(b["p1"][1])), width=float(b["width"]),
               bones=int(b.get("bones", 2)))
    if "pivot_pixel" in b:
        out["pivot_pixel"] = (int(b["pivot_pixel"][0]), int(b["pivot_pixel"][1]))
    return out


def _check_camera_entry(where, t):
    """The optional "camera" of one transforms.json entry (not in the reference; camera moves): a dict {"rot_angle" (degrees,
    default 0), "rot_axis" (3 numbers, default the Y axis, not zero), "translation" (3 numbers, default 0), "pivot" (3 numbers:
    a point in the coordinates of depth_to_world_coords) or "pivot_pixel" ([x, y]: the point of that pixel, resolved with
    depth_transform.pivot_at_pixel when the edit runs)} -- the motion of the CAMERA.  ValueError naming `where`."""
    if not isinstance(t, dict) or "camera" not in t:
        return
    cam = t["camera"]
    if not isinstance(cam, dict):
        raise ValueError(f"{where}: \"camera\" must be an object with {CAMERA_KEYS}, got {cam!r}")
    extra = [k for k in cam if k not in CAMERA_KEYS]
    if extra:
        raise ValueError(f"{where}: \"camera\" has unknown keys {extra} (known: {CAMERA_KEYS})")
    f32 = lambda v: float(np.float32(v))
    with np.errstate(over="ignore"):
        if "rot_angle" in cam and not (_is_number(cam["rot_angle"]) and np.isfinite(f32(cam["rot_angle"]))):
            raise ValueError(f"{where}: \"camera\": \"rot_angle\" must be a finite number, got {cam['rot_angle']!r}")
        for key in ("rot_axis", "translation", "pivot"):
            if key in cam:
                v = cam[key]
                if not isinstance(v, (list, tuple)) or len(v) != 3 or not all(_is_number(x) for x in v) or \
                        not all(np.isfinite(f32(x)) for x in v):
                    raise ValueError(f"{where}: \"camera\": \"{key}\" must be a list of 3 finite numbers, got {v!r}")
        if "rot_axis" in cam and not any(f32(x) != 0.0 for x in cam["rot_axis"]):
            raise ValueError(f"{where}: \"camera\": \"rot_axis\" must not be zero")
    if "pivot_pixel" in cam:
        v = cam["pivot_pixel"]
        if "pivot" in cam:
            raise ValueError(f"{where}: \"camera\" has both \"pivot\" and \"pivot_pixel\"")
        if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(isinstance(x, int) and not isinstance(x, bool) and x >= 0 for x in v):
            raise ValueError(f"{where}: \"camera\": \"pivot_pixel\" must be [x, y], two integers >= 0, got {v!r}")


def camera_args(t):
    """The "camera" of one transforms.json entry -> None (no key), or dict(rot_angle, rot_axis, translation) with `pivot` (three
    floats) or `pivot_pixel` ((x, y), to resolve with depth_transform.pivot_at_pixel) when the entry gives one."""
    if not isinstance(t, dict) or "camera" not in t:
        return None
    _check_camera_entry("camera_args", t)
    cam = t["camera"]
    out = dict(rot_angle=float(cam.get("rot_angle", 0.0)), rot_axis=tuple(float(v) for v in cam.get("rot_axis", [0.0, 1.0, 0.0])),
               translation=tuple(float(v) for v in cam.get("translation", [0.0, 0.0, 0.0])))
    if "pivot" in cam:
        out["pivot"] = tuple(float(v) for v in cam["pivot"])
    if "pivot_pixel" in cam:
        out["pivot_pixel"] = (int(cam["pivot_pixel"][0]), int(cam["pivot_pixel"][1]))
    return out


def is_pure_camera(t):
    """An entry with "camera" and no transform key: a pure camera move of the whole image."""
    return isinstance(t, dict) and "camera" in t and not any(k in t for k in _TRANSFORM_KEYS)


def _check_similarity_entries(scene_dir, transforms):
    """Every entry of transforms.json, and every member of its "objects" list."""
    for name, t in transforms.items():
        _check_camera_entry(f"{scene_dir}: transform {name!r}", t)
        if isinstance(t, dict) and isinstance(t.get("objects"), (list, tuple)):
            for m, o in enumerate(t["objects"]):
                if isinstance(o, dict) and "camera" in o:
                    raise ValueError(f"{scene_dir}: transform {name!r}, object {m}: \"camera\" belongs to the entry, not to a "
                                     "member of \"objects\"")
        if isinstance(t, dict) and "remove" in t and "objects" in t:
            raise ValueError(f"{scene_dir}: transform {name!r}: \"remove\" belongs inside a member of \"objects\"")
        _check_similarity_entry(f"{scene_dir}: transform {name!r}", t)
        _check_bend_entry(f"{scene_dir}: transform {name!r}", t)
        if isinstance(t, dict) and isinstance(t.get("objects"), (list, tuple)):
            for m, o in enumerate(t["objects"]):
                _check_similarity_entry(f"{scene_dir}: transform {name!r}, object {m}", o)
                _check_bend_entry(f"{scene_dir}: transform {name!r}, object {m}", o)


def load_scene_geometry(scene_dir, img_res=512):
    """The geometric inputs of a scene only -- what `transform_depth` needs (test/test_diffusion_handles.py:213-215, 247-261):
    dict(transforms, fg_mask [1,1,R,R] in {0,1}, depth [1,1,R,R], bg_depth [1,1,R,R]).  Needs transforms.json, mask.png,
    depth.exr / .npy, bg_depth.exr / .npy; no image, no prompt.
    A scene with a mask_0.png is a multi-object scene (not in the reference): its masks are mask_0.png .. mask_{M-1}.png
    (consecutive, 1 <= M <= 8, each read like mask.png; a mask.png beside them is not read), bg_depth is the depth with all of
    them removed, and every transforms.json entry is {"objects": [M ordinary entries], "object_weights": "equal" | [M floats]
    (optional)} (object_transform_args).  The dict then also has fg_masks, the list of the M masks, and fg_mask is their union.
    An ordinary entry may also carry "scale" (a positive number, or 3 along the camera axes) and "pivot" (3 numbers, a point in
    the coordinates of depth_to_world_coords) (not in the reference; transform_args); malformed values raise ValueError naming
    the scene and the entry here, when the scene is loaded.
    A member of "objects" may carry "mask": m (not in the reference; copies of an object): it is then one more INSTANCE of mask
    m, and the list may be longer than the number of masks (at most 8, every mask drawn by some member; members without "mask"
    keep their own position's mask).  "object_weights" then has one entry per member.  Lists without any "mask" give exactly
    what they gave before.
    A member of "objects" may be {"remove": true} (not in the reference; object removal): it deletes the mask of its own position
    -- it carries no transform key and no "mask", and no other member may name its mask; "object_weights" lists have one entry
    per remaining member.  In a single-mask scene the entry {"remove": true} deletes the one object.  bg_depth has the removed
    objects removed, as it has all objects.  Files without "remove" load to exactly what they loaded to.
    A scene directory may hold donor/ (not in the reference; object insertion): depth.exr / .npy and mask_0.png .. mask_{D-1}.png
    of a SECOND image (and, for load_scene, its input.png and prompt.txt).  The dict then also has donor = dict(depth, masks).
    A member of "objects" may carry "donor": d: it is an instance of donor mask d, stands behind the host's members, carries
    no "mask" and no "remove", and an entry with donor members draws every donor mask (entry_donor).  The depth scale between
    the two images is not estimated: the member's "scale" brings it.  Files without the key load to what they loaded to.
    An entry may carry "camera": {"rot_angle", "rot_axis", "translation", "pivot" | "pivot_pixel": [x, y]} (not in the reference;
    camera moves, _check_camera_entry): the edit also moves the viewpoint.  In a multi-object scene it stands beside "objects";
    in a single-mask scene an entry with only "camera" is a pure camera move of the whole image.  Malformed values raise
    ValueError here, when the scene is loaded; files without the key load to what they loaded to.
    A member of "objects" -- in a single-mask scene the entry itself -- may carry "bend": {"p0", "p1", "width", "bones",
    "pivot_pixel"} (not in the reference; bend edits, _check_bend_entry): the object bends across the line p0 p1, its own
    rotation_angle / rotation_axis / translation being the full motion of the far side (depth_transform.bend_chain).
    Malformed values raise ValueError here; files without the key load to what they loaded to."""
    import torch
    j = os.path.join
    with open(j(scene_dir, "transforms.json")) as f:
        transforms = json.load(f, object_pairs_hook=OrderedDict)
    _check_similarity_entries(scene_dir, transforms)

    def mask_of(name):
        mask = load_image(j(scene_dir, name))[None]
        if mask.shape[1] > 1:
            mask = mask.mean(dim=1, keepdim=True)
        return (crop_and_resize(mask, img_res) > 0.5).to(torch.float32)

    n_donor = 0
    while os.path.exists(j(scene_dir, "donor", f"mask_{n_donor}.png")):
        n_donor += 1
    if os.path.isdir(j(scene_dir, "donor")) and n_donor == 0:
        raise ValueError(f"{scene_dir}: donor/ holds no mask_0.png")
    if n_donor > MAX_SCENE_OBJECTS:
        raise ValueError(f"{scene_dir}: {n_donor} donor masks, at most {MAX_SCENE_OBJECTS} are supported")
    masks = None
    if os.path.exists(j(scene_dir, "mask_0.png")):
        M = 1
        while os.path.exists(j(scene_dir, f"mask_{M}.png")):
            M += 1
        if M > MAX_SCENE_OBJECTS:
            raise ValueError(f"{scene_dir}: {M} object masks, at most {MAX_SCENE_OBJECTS} are supported")
        _check_object_entries(scene_dir, transforms, M, n_donor)
        masks = [mask_of(f"mask_{m}.png") for m in range(M)]
        union = masks[0] != 0
        for m in masks[1:]:
            union = union | (m != 0)
        mask = union.to(torch.float32)
    else:
        _check_object_entries(scene_dir, transforms, 0, n_donor)
        mask = mask_of("mask.png")

    def depth_of(stem):
        if os.path.exists(j(scene_dir, stem + ".exr")):
            d = read_depth_exr(j(scene_dir, stem + ".exr"))
        elif os.path.exists(j(scene_dir, stem + ".npy")):
            d = np.load(j(scene_dir, stem + ".npy")).astype(np.float32)
        else:
            raise FileNotFoundError(j(scene_dir, stem + ".exr"))
        return crop_and_resize(torch.from_numpy(np.ascontiguousarray(d))[None, None], img_res).to(torch.float32)

    geo = dict(transforms=transforms, fg_mask=mask, depth=depth_of("depth"), bg_depth=depth_of("bg_depth"))
    if masks is not None:
        geo["fg_masks"] = masks
    if n_donor:
        geo["donor"] = dict(depth=depth_of(j("donor", "depth")), masks=[mask_of(j("donor", f"mask_{d}.png")) for d in range(n_donor)])
    return geo


def load_scene(scene_dir, img_res=512):
    """`load_diffhandles_inputs` (test/test_diffusion_handles.py:208-263) -> dict(transforms, prompt, img [1,3,R,R],
    fg_mask [1,1,R,R] in {0,1}, depth [1,1,R,R], bg_depth [1,1,R,R]); a multi-object scene also has fg_masks
    (load_scene_geometry)."""
    j = os.path.join
    with open(j(scene_dir, "prompt.txt")) as f:
        lines = [ln for ln in f.read().splitlines() if len(ln) > 0]
    if not lines:
        raise ValueError(f"{scene_dir}: empty prompt")
    img = load_image(j(scene_dir, "input.png"))[None]
    img = crop_and_resize(img[:, :3], img_res)
    geo = load_scene_geometry(scene_dir, img_res)
    sc = dict(transforms=geo["transforms"], prompt=lines[0], img=img, fg_mask=geo["fg_mask"], depth=geo["depth"],
              bg_depth=geo["bg_depth"])
    if "fg_masks" in geo:          # a multi-object scene (load_scene_geometry)
        sc["fg_masks"] = geo["fg_masks"]
    if "donor" in geo:             # the second image of an insertion: its own picture and prompt beside its depth and masks
        with open(j(scene_dir, "donor", "prompt.txt")) as f:
            lines = [ln for ln in f.read().splitlines() if len(ln) > 0]
        if not lines:
            raise ValueError(f"{scene_dir}: donor: empty prompt")
        dimg = crop_and_resize(load_image(j(scene_dir, "donor", "input.png"))[None][:, :3], img_res)
        sc["donor"] = dict(geo["donor"], img=dimg, prompt=lines[0])
    return sc


def transform_args(t):
    """One transforms.json entry -> keyword arguments of `transform_foreground` (test_diffusion_handles.py:137-150).  `scale`
    (a float or three) / `pivot` (three floats) only when the entry has "scale" / "pivot" (not in the reference).  The entry
    {"remove": true} (object removal) gives dict(remove=True) and nothing else."""
    import torch
    if _is_removal(t):          # a single-mask scene's {"remove": true}: the edit deletes the object (no transform)
        if t["remove"] is not True or len(t) != 1:
            raise ValueError(f"transform_args: an entry that removes the object is exactly {{\"remove\": true}}, got {dict(t)!r}")
        return dict(remove=True)
    _check_similarity_entry("transform_args", t)
    _check_bend_entry("transform_args", t)
    if is_pure_camera(t):       # a pure camera move of the whole image: no object transform
        return dict(camera=camera_args(t), camera_only=True)
    args = dict(rot_angle=float(t.get("rotation_angle", 0.0)),
                rot_axis=torch.tensor(t.get("rotation_axis", [0.0, 1.0, 0.0]), dtype=torch.float32),
                translation=torch.tensor(t.get("translation", [0.0, 0.0, 0.0]), dtype=torch.float32))
    if "scale" in t:
        args["scale"] = float(t["scale"]) if _is_number(t["scale"]) else tuple(float(v) for v in t["scale"])
    if "pivot" in t:
        args["pivot"] = tuple(float(v) for v in t["pivot"])
    if isinstance(t, dict) and "camera" in t:
        args["camera"] = camera_args(t)
    if isinstance(t, dict) and "bend" in t:          # (not in the reference) the entry's motion is a bend chain's full motion
        args["bend"] = bend_args(t)
    return args


def object_transform_args(entry):
    """One transforms.json entry of a multi-object scene, {"objects": [t_0 .. t_{M-1}], "object_weights": "equal" | [w ..]} ->
    the `transforms` / `object_weights` keyword arguments of `transform_foreground_objects`: M (rot_angle, rot_axis,
    translation) triples in mask order (`{}` leaves an object in place) and None, "equal" or a list of floats.  An object
    whose entry has "scale" or "pivot" gives the 5-tuple (rot_angle, rot_axis, translation, scale, pivot) instead.  When a
    member carries "mask" (entry_instances) the dict also has `instances`, the mask index of every member.  When a member is
    {"remove": true} (entry_removal) the dict also has `remove`, the mask indices the edit deletes; transforms, weights and
    `instances` then speak about the remaining members and the remaining masks.  When a member carries "donor" (entry_donor)
    the dict also has `donor`, the donor mask index of every donor member: `transforms` and the weights list the host's
    (remaining) members and then the donor's, and `instances` is always there -- the host's table (or 0, 1, ...), then
    M' + d for a member of donor mask d, M' the number of (remaining) host masks.  When a member carries "bend" (bend_args) the
    dict also has `bends`, one entry per transform: None, or the member's bend_args -- the caller replaces that transform by
    depth_transform.bend_chain of its angle, axis, translation and pivot (tools/run_edit.py)."""
    if not isinstance(entry, dict) or "objects" not in entry:
        raise ValueError("object_transform_args: the entry has no \"objects\" list")
    if "camera" in entry:          # camera moves: the entry's camera beside what the entry gives without it
        rest = OrderedDict((k, v) for k, v in entry.items() if k != "camera")
        return dict(object_transform_args(rest), camera=camera_args(entry))
    dn = entry_donor(entry["objects"], None, "object_transform_args")
    if dn is not None:
        host, members, index = dn
        out = object_transform_args({"objects": host}) if host else dict(transforms=[], object_weights=None)
        n_host = max(out["instances"]) + 1 if "instances" in out else len(out["transforms"])
        more = object_transform_args({"objects": members})
        if "bends" in out or "bends" in more:
            out["bends"] = out.get("bends", [None] * len(out["transforms"])) + more.get("bends", [None] * len(more["transforms"]))
        out["transforms"] = out["transforms"] + more["transforms"]
        out["instances"] = out.get("instances", list(range(n_host))) + [n_host + d for d in index]
        w = entry.get("object_weights")
        out["object_weights"] = w if w is None or isinstance(w, str) else [float(v) for v in w]
        out["donor"] = index
        return out
    rem = entry_removal(entry["objects"], None, "object_transform_args")
    members = entry["objects"] if rem is None else rem[1]
    triples, bends = [], []
    for t in members:
        a = transform_args(t)
        triple = (a["rot_angle"], a["rot_axis"], a["translation"])
        triples.append(triple + (a.get("scale"), a.get("pivot")) if "scale" in a or "pivot" in a else triple)
        bends.append(a.get("bend"))
    bent = {} if all(b is None for b in bends) else dict(bends=bends)
    w = entry.get("object_weights")
    if w is not None and not isinstance(w, str):
        w = [float(v) for v in w]
    if rem is not None:          # `remove`: the scene's mask indices the edit deletes; `instances` counts among the remaining masks
        return dict(transforms=triples, object_weights=w, remove=rem[0], **({} if rem[2] is None else dict(instances=rem[2])), **bent)
    inst = entry_instances(entry["objects"], None, "object_transform_args")
    return dict(transforms=triples, object_weights=w, **({} if inst is None else dict(instances=inst)), **bent)
