"""CPU: the argument record of the re-projection (dh_reproject_args, _lib.ReprojectArgs; DESIGN.md "One record for the
re-projection").  Host only, no GPU: the layout of the ctypes twin against the library's own reading of the struct; the record
query against every pinned size of the positional queries; and the refusals, which precede any launch -- the record entry, the
positional entry and the parent commit's library say the same words."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_arena_hooks as AH  # noqa: E402  (helpers only: the fixture, the pinned sizes, the logged query)
import test_bend_ref as TB  # noqa: E402  (its pinned sizes only)
import test_view_surfaces_ref as TV  # noqa: E402  (its pinned sizes only)
from diffusionhandles_amd import _lib  # noqa: E402

L = AH.L
Args = _lib.ReprojectArgs
I32P, U8P, F64P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_double)


# ---- 1. layout -------------------------------------------------------------------------------------------------------------------
def _dump(lib, a):
    n = ctypes.c_int(0)
    out = (ctypes.c_int64 * 64)()
    assert lib.dh_dbg_reproject_args(ctypes.byref(a), out, 64, ctypes.byref(n)) == 0, lib.dh_last_error()
    return list(out[:n.value])


def test_the_ctypes_twin_has_the_layout_the_library_reads(L):
    a = Args()
    want = []
    for k, (name, ctype) in enumerate(Args._fields_):
        if name == "struct_bytes":
            want.append(ctypes.sizeof(Args))
            continue
        if ctype is ctypes.c_float:
            v = 1.5 + k
            bits = struct.unpack("<I", struct.pack("<f", v))[0]
        elif ctype is ctypes.c_double:
            v = 2.25 + k
            bits = struct.unpack("<q", struct.pack("<d", v))[0]
        elif ctype in (ctypes.c_int32, ctypes.c_size_t):
            v = bits = 1000 + k
        else:                                                   # a pointer: a distinct address, never followed
            bits = 0x10000 + 64 * k
            v = ctypes.c_void_p(bits) if ctype is ctypes.c_void_p else ctypes.cast(ctypes.c_void_p(bits), ctype)
        setattr(a, name, v)
        want.append(bits)
    assert len(set(want)) == len(want) == len(Args._fields_)
    assert _dump(L, a) == want
    # a new record is zero beyond struct_bytes: zero means off
    assert _dump(L, Args()) == [ctypes.sizeof(Args)] + [0] * (len(Args._fields_) - 1)


@pytest.mark.parametrize("wrong", [0, 8, ctypes.sizeof(Args) - 8, ctypes.sizeof(Args) + 8])
def test_a_wrong_struct_bytes_is_refused_before_anything_is_read(L, wrong):
    a = Args(res=64, n_fg=100, n_edits=1, n_objects=1)
    nb = ctypes.c_size_t(7)
    assert L.dh_reproject_workspace(ctypes.byref(a), ctypes.byref(nb)) == 0 and nb.value > 7
    a.struct_bytes = wrong
    nb = ctypes.c_size_t(7)
    assert L.dh_reproject_workspace(ctypes.byref(a), ctypes.byref(nb)) == -1 and nb.value == 7
    assert L.dh_last_error() == b"dh_reproject_workspace: struct_bytes is not sizeof(dh_reproject_args)"
    assert L.dh_reproject(ctypes.byref(a)) == -1
    assert L.dh_last_error() == b"dh_reproject: struct_bytes is not sizeof(dh_reproject_args)"
    assert L.dh_reproject(None) == -1 and L.dh_reproject_workspace(None, ctypes.byref(nb)) == -1 and nb.value == 7


# ---- 2. sizes --------------------------------------------------------------------------------------------------------------------
def _ones(n):
    return np.ones(n, dtype=np.uint8)


def _query_record(name, args):
    """The record the positional query `name` fills from `args` (csrc/reproject_compat.cpp), and the host array it points into.
    A query that reserved view rows whatever the call would bring is a view in every edit."""
    views = None
    if name == "dh_reproject_workspace_bytes":
        a = Args(res=args[0], n_fg=args[1], n_edits=args[2], n_objects=1)
    elif name == "dh_reproject_objects_workspace_bytes":
        a = Args(res=args[0], n_fg=args[1], n_edits=args[2], n_objects=args[3])
    elif name == "dh_reproject_footprints_workspace_bytes":
        a = Args(res=args[0], n_fg=args[1], n_edits=args[2], n_objects=args[3], footprints=args[4])
    elif name in ("dh_reproject_instances_workspace_bytes", "dh_reproject_donor_workspace_bytes", "dh_reproject_camera_workspace_bytes"):
        a = Args(res=args[0], n_fg=args[1], n_edits=args[2], n_objects=args[3], n_instances=args[4], footprints=args[5])
        views = _ones(args[2]) if "camera" in name else None
    elif name == "dh_reproject_surface_ws_bytes":
        a = Args(res=args[0], n_fg=args[1], n_edits=args[2], n_objects=args[3], n_instances=args[4], view_surfaces=args[5])
        views = _ones(args[2])
    elif name == "dh_reproject_bend_ws_bytes":
        a = Args(res=args[0], n_fg=args[1], n_edits=args[2], n_objects=args[3], n_instances=args[4], view_surfaces=args[5],
                 footprints=args[6], n_bones=args[7])
        views = _ones(args[2])
    elif name == "dh_reproject_background_workspace_bytes":
        a = Args(res=args[0], n_fg=0, n_edits=1)
    elif name == "dh_reproject_surface_background_ws_bytes":
        a = Args(res=args[0], n_fg=0, n_edits=1, view_surfaces=args[1])
        views = _ones(1)
    else:
        raise AssertionError(name)
    if views is not None:
        a.has_view = views.ctypes.data_as(U8P)
    return a, views


def _logged_record(lib, a):
    assert lib.dh_dbg_arena_log(1) == 0
    nb = ctypes.c_size_t()
    assert lib.dh_reproject_workspace(ctypes.byref(a), ctypes.byref(nb)) == 0, lib.dh_last_error()
    n = ctypes.c_int(0)
    assert lib.dh_dbg_arena_log_read(None, 0, ctypes.byref(n)) == 0
    out = (ctypes.c_int64 * (3 * max(n.value, 1)))()
    assert lib.dh_dbg_arena_log_read(out, n.value, ctypes.byref(n)) == 0
    assert lib.dh_dbg_arena_log(0) == 0
    return nb.value, [tuple(out[3 * i + 1:3 * i + 3]) for i in range(n.value)]


PINNED = [(name, args, size) for name, rows in AH.PARENT_SIZES.items() if name.startswith("dh_reproject_") for args, size in rows] + \
    TV.SURFACE_CASES + [("dh_reproject_bend_ws_bytes", args, size) for args, size in TB.BEND_SIZES]


def test_the_pinned_rows_are_all_here():
    names = {n for n, _, _ in PINNED}
    assert names == {n for n in list(AH.PARENT_SIZES) + list(TV.SURFACE_SIZES) if n.startswith("dh_reproject_")} | {"dh_reproject_bend_ws_bytes"}
    assert len(PINNED) == 27 + 10 + 4


@pytest.mark.parametrize("name,args,size", PINNED, ids=[f"{n[3:]}{a}" for n, a, _ in PINNED])
def test_the_record_query_answers_every_pinned_size(L, name, args, size):
    a, keep = _query_record(name, args)
    got, takes = _logged_record(L, a)
    assert got == size
    # ... with the takes of the positional query, one for one
    _, old = AH._logged(L, name, args)
    assert takes == [(off, nbytes) for _, off, nbytes in old]


def _packed(takes):
    """the answer for a list of take sizes: each at the next multiple of 256, and 256 behind the last"""
    end = 0
    for nbytes in takes:
        end = (end + 255) // 256 * 256 + nbytes
    return end + 256


@pytest.mark.parametrize("args,size", TB.BEND_SIZES, ids=[str(a) for a, _ in TB.BEND_SIZES])
def test_a_bend_record_without_a_view_takes_no_view_rows(L, args, size):
    """The bend query reserved the view rows for every call; the record knows whether an edit has a view.  Without one the answer
    is the pinned size minus exactly the take of the view rows (n_edits rows of 128 bytes) as the arena log reports it -- and,
    where the setting was on, minus the takes of the view surfaces, which act only where there is a view."""
    with_view, keep = _query_record("dh_reproject_bend_ws_bytes", args)
    pinned, full = _logged_record(L, with_view)
    assert pinned == size
    a, _ = _query_record("dh_reproject_bend_ws_bytes", args)
    a.has_view = None
    got, takes = _logged_record(L, a)
    K, surfaces, footprints = args[2], args[5], args[6]
    n_base = 21 + (4 if footprints else 0)                        # (the carving every call has, then the footprints' four)
    assert full[n_base][1] == K * 128 and len(full) == n_base + 1 + (4 if surfaces else 0)          # the view rows, then the surfaces' four
    assert [n for _, n in takes] == [n for _, n in full[:n_base]]
    assert got == _packed([n for _, n in full[:n_base]]) < pinned
    if not surfaces:
        assert pinned - got == (full[n_base][0] + full[n_base][1]) - (full[n_base - 1][0] + full[n_base - 1][1])
    # a record with a view in one edit of several reserves them as the pinned query did
    if K > 1:
        one = np.zeros(K, dtype=np.uint8)
        one[K - 1] = 1
        a.has_view = one.ctypes.data_as(U8P)
        assert _logged_record(L, a) == (pinned, full)


def test_the_record_query_sums_the_points_over_the_instances(L):
    """with both tables the query counts n_pts as the call does; a table that names a mask outside the list is refused"""
    obj_start = np.asarray([0, 300, 900], dtype=np.int32)
    inst_obj = np.asarray([1, 0, 1], dtype=np.int32)
    a = Args(res=64, n_fg=900, n_edits=3, n_objects=2, n_instances=3)
    a.obj_start, a.inst_obj = obj_start.ctypes.data_as(I32P), inst_obj.ctypes.data_as(I32P)
    b = Args(res=64, n_fg=1500, n_edits=3, n_objects=2, n_instances=3)
    assert _logged_record(L, a) == _logged_record(L, b)
    assert _logged_record(L, a)[0] == AH._query(L, "dh_reproject_instances_workspace_bytes", (64, 1500, 3, 2, 3, 0))
    inst_obj[2] = 2
    nb = ctypes.c_size_t(7)
    assert L.dh_reproject_workspace(ctypes.byref(a), ctypes.byref(nb)) == -1 and nb.value == 7
    assert L.dh_last_error() == b"dh_reproject_workspace: inst_obj: an instance names a mask outside 0 .. n_objects - 1"


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------
# One malformed call per shared check of the object function, in the order it makes them.  Every call here is ALSO given a
# workspace of 16 bytes, so a case that failed to trip its own check would end at "workspace too small", the last refusal before
# the first launch: nothing here can start device work, with or without a GPU.
RES, N_FG, K, M = 64, 10, 2, 2
PTR = 0x7000                     # stands for every device pointer (16-byte aligned); never followed before a launch


def _rows(n, **bad):
    rows = np.zeros((n, 16), dtype=np.float64)
    rows[:, 0], rows[:, 3], rows[:, 8:11] = 1.0, 1.0, 1.0
    for k, v in bad.items():
        rows[n - 1, int(k[1:])] = v
    return rows


def _base():
    return dict(n_fg=N_FG, n_objects=M, obj_start=[0, 4, 10], res=RES, n_edits=K, rows=_rows(K * 2), footprints=0, max_ratio=0.0,
                corr_capacity=N_FG, n_instances=2, inst_obj=[0, 1], corr_inst=PTR, donor_depth=0, n_host_objects=M, views=None, has_view=None,
                bg=PTR, infill_border=0, view_surfaces=0, surface_max_ratio=0.0, n_bones=1, bone_w=0, depth=PTR, out=PTR)


VIEWS = _rows(K)
VIEWS[:, 14] = 1.0
BAD_VIEW = VIEWS.copy()
BAD_VIEW[1, 9] = -1.0
# (what to change, the parent library's text: written down once from the build of the parent commit, through the positional entry)
REFUSALS = [
    (dict(n_bones=5), "reproject_instances: n_bones must lie in 1 .. 4"),
    (dict(n_bones=2), "reproject_instances: n_bones > 1 without bone_w"),
    (dict(n_bones=2, bone_w=PTR + 4, rows=_rows(K * 2 * 2)), "reproject_instances: bone_w must be 16-byte aligned"),
    (dict(view_surfaces=2), "reproject_instances: view_surfaces must be 0 or 1"),
    (dict(view_surfaces=1, surface_max_ratio=1.0), "reproject_instances: surface_max_ratio must be 0 (none) or finite and > 1"),
    (dict(surface_max_ratio=1.5), "reproject_instances: surface_max_ratio without view_surfaces"),
    (dict(view_surfaces=1, footprints=1),
     "reproject_instances: view_surfaces with footprints are not supported (footprints stay refused with a view)"),
    (dict(depth=0), "reproject_instances: null input"),
    (dict(out=0), "reproject_instances: null output"),
    (dict(res=1), "reproject_instances: bad sizes"),
    (dict(n_objects=9, n_host_objects=9), "reproject_instances: 1 to 8 objects"),
    (dict(n_instances=9), "reproject_instances: 1 to 8 instances"),
    (dict(footprints=2), "reproject_instances: footprints must be 0 or 1"),
    (dict(n_host_objects=3), "reproject_instances: n_host_objects must lie in 0 .. n_objects"),
    (dict(n_host_objects=1), "reproject_instances: donor objects without a donor depth"),
    (dict(n_host_objects=1, donor_depth=PTR, footprints=1, corr_capacity=RES * RES),
     "reproject_instances: footprints with a donor are not supported (two images share pixel indices)"),
    (dict(n_host_objects=1, donor_depth=PTR, corr_inst=0), "reproject_instances: a donor needs the instance column (corr_inst)"),
    (dict(n_host_objects=1, donor_depth=PTR, view_surfaces=1),
     "reproject_instances: view_surfaces with a donor are not supported (two images share pixel indices)"),
    (dict(footprints=1, max_ratio=0.5), "reproject_instances: footprint max_ratio must be 0 (none) or finite and > 1"),
    (dict(max_ratio=1.5), "reproject_instances: footprint max_ratio without footprints"),
    (dict(obj_start=[0, 4, 9]), "reproject_instances: obj_start must run from 0 to n_fg"),
    (dict(obj_start=[0, 0, 10]), "reproject_instances: obj_start must increase (no empty object)"),
    (dict(inst_obj=[0, 2]), "reproject_instances: inst_obj: an instance names a mask outside 0 .. n_objects - 1"),
    (dict(inst_obj=[0, 0]), "reproject_instances: inst_obj: a mask without an instance (removing an object is not supported)"),
    (dict(res=46341), "reproject_instances: res * res + n_pts does not fit the int owner map"),
    (dict(corr_capacity=N_FG - 1),
     "reproject_instances: correspondence capacity too small (n_fg rows per edit without footprints, res * res with)"),
    (dict(rows=_rows(K * 2, c8=0.0)), "reproject_instances: transform row: the scale must be positive and finite"),
    (dict(rows=_rows(K * 2, c12=float("inf"))), "reproject_instances: transform row: the pivot must be finite"),
    (dict(rows=_rows(K * 2, c14=0.5)), "reproject_instances: transform row: the has-pivot flag must be 0 or 1"),
    (dict(views=BAD_VIEW, has_view=[0, 1]),
     "reproject_instances: view row: malformed (finite members, scale positive, has-pivot flag 0 or 1)"),
    (dict(views=VIEWS, has_view=[1, 0], footprints=1, corr_capacity=RES * RES), "reproject_instances: footprints with a view are not supported"),
    (dict(views=VIEWS, has_view=[1, 0], bg=0), "reproject_instances: a view needs bg_valid, bg_corr and bg_counts"),
    (dict(views=VIEWS, has_view=[0, 1], view_surfaces=1),
     "reproject_instances: correspondence capacity too small (res * res rows per edit with view surfaces)"),
    (dict(), "reproject_instances: workspace too small"),
]
# the checks the widest positional entry makes itself, ahead of the shared ones: the words are the parent's, the name its own
SHIM_REFUSALS = [
    (dict(infill_border=2), "infill_border must be 0 (zero) or 1 (reflect)"),
    (dict(n_host_objects=-1), "n_host_objects must lie in 0 .. n_objects"),
    (dict(n_edits=0), "bad sizes"),
]


def _host(d):
    """the host arrays of a call (kept alive by the caller)"""
    h = dict(obj_start=np.asarray(d["obj_start"], dtype=np.int32), inst_obj=np.asarray(d["inst_obj"], dtype=np.int32), rows=d["rows"],
             views=d["views"], has_view=None if d["has_view"] is None else np.asarray(d["has_view"], dtype=np.uint8))
    as_p = lambda arr, t: None if arr is None else arr.ctypes.data_as(t)
    return h, (as_p(h["obj_start"], I32P), as_p(h["inst_obj"], I32P), as_p(h["rows"], F64P), as_p(h["views"], F64P), as_p(h["has_view"], U8P))


def _positional(lib, d):
    h, (obj_start, inst_obj, rows, views, has_view) = _host(d)
    p, o, bg = d["depth"], d["out"], d["bg"]
    rc = lib.dh_reproject_bend_edits(p, p, p, d["n_fg"], d["n_objects"], obj_start, d["res"], p, p, 1.0, 1.0, 1.0, 1.0, d["n_edits"], rows,
                                     None, o, o, o, o, o, o, o, o, PTR, 16, None, d["footprints"], d["max_ratio"], d["corr_capacity"],
                                     d["n_instances"], inst_obj, d["corr_inst"], d["donor_depth"], d["n_host_objects"], views, has_view,
                                     bg, bg, bg, d["infill_border"], d["view_surfaces"], d["surface_max_ratio"], d["n_bones"], d["bone_w"])
    return rc, lib.dh_last_error().decode()


def _record(lib, d):
    h, (obj_start, inst_obj, rows, views, has_view) = _host(d)
    p, o, bg = d["depth"], d["out"], d["bg"]
    a = Args(res=d["res"], n_fg=d["n_fg"], n_objects=d["n_objects"], n_edits=d["n_edits"], n_instances=d["n_instances"],
             n_bones=d["n_bones"], corr_capacity=d["corr_capacity"], footprints=d["footprints"],
             n_donor_objects=d["n_objects"] - d["n_host_objects"], infill_border=d["infill_border"], view_surfaces=d["view_surfaces"],
             max_ratio=d["max_ratio"], surface_max_ratio=d["surface_max_ratio"], inv_fx=1.0, inv_fy=1.0, fx=1.0, fy=1.0,
             depth=p, bg_depth=p, fg_pix=p, grid_x=p, grid_y=p, donor_depth=d["donor_depth"], bg_valid=bg, bone_w=d["bone_w"],
             zmap=o, raw_mask=o, clean_mask=o, disparity=o, vis=o, target_xy=o, corr=o, corr_inst=d["corr_inst"], counts=o,
             bg_corr=bg, bg_counts=bg, workspace=PTR, workspace_bytes=16)
    a.obj_start, a.inst_obj, a.xforms_host, a.views, a.has_view = obj_start, inst_obj, rows, views, has_view
    rc = lib.dh_reproject(ctypes.byref(a))
    return rc, lib.dh_last_error().decode()


@pytest.mark.parametrize("change,parent", REFUSALS, ids=[t.split(": ", 1)[1][:48] for _, t in REFUSALS])
def test_a_refusal_is_the_parents_by_either_entry(L, change, parent):
    d = dict(_base(), **change)
    assert _positional(L, d) == (-1, parent)
    assert _record(L, d) == (-1, parent)


@pytest.mark.parametrize("change,words", SHIM_REFUSALS, ids=[w[:32] for _, w in SHIM_REFUSALS])
def test_a_check_of_the_positional_entry_keeps_its_words_and_its_place(L, change, words):
    """made by dh_reproject_bend_edits itself ahead of everything shared (here: ahead of a bad n_bones, the first shared check),
    under its own name; the record entry says the same words where the shared checks reach them"""
    d = dict(_base(), n_bones=5, **change)
    assert _positional(L, d) == (-1, "dh_reproject_bend_edits: " + words)
    rc, text = _record(L, dict(_base(), **change))
    assert rc == -1 and text.split(": ", 1)[1] == words


def test_the_call_without_a_foreground_point_refuses_as_its_entry_did(L):
    """n_fg = 0: the record entry is dh_reproject_surface_background's sequence, and says so"""
    a = Args(res=64, n_fg=0, n_edits=1, bg_depth=PTR, grid_x=PTR, grid_y=PTR, zmap=PTR, disparity=PTR, counts=PTR, workspace=PTR,
             workspace_bytes=16)
    for change, text in ((dict(infill_border=3), "infill_border must be 0 (zero) or 1 (reflect)"), (dict(view_surfaces=2), "view_surfaces must be 0 or 1"),
                         (dict(surface_max_ratio=2.0), "surface_max_ratio without view_surfaces"), (dict(bg_depth=0), "null input"),
                         (dict(zmap=0), "null output"), (dict(res=40000), "bad sizes"), (dict(n_edits=2), "the call without a foreground point takes one edit"),
                         (dict(), "workspace too small")):
        b = Args.from_buffer_copy(a)
        for k, v in change.items():
            setattr(b, k, v)
        assert L.dh_reproject(ctypes.byref(b)) == -1
        assert L.dh_last_error().decode() == "dh_reproject_surface_background: " + text
    one, view = _ones(1), BAD_VIEW[1:].copy()
    a.has_view, a.views = one.ctypes.data_as(U8P), view.ctypes.data_as(F64P)
    assert L.dh_reproject(ctypes.byref(a)) == -1
    assert L.dh_last_error().decode() == "dh_reproject_surface_background: view row: malformed (finite members, scale positive, has-pivot flag 0 or 1)"
    a.views = VIEWS.ctypes.data_as(F64P)
    assert L.dh_reproject(ctypes.byref(a)) == -1
    assert L.dh_last_error().decode() == "dh_reproject_surface_background: a view needs bg_valid, bg_corr and bg_counts"
    # the positional entries say the same: the words above are theirs
    assert L.dh_reproject_surface_background(PTR, 64, PTR, PTR, 1.0, 1.0, 1.0, 1.0, None, PTR, PTR, PTR, PTR, 16, None, view.ctypes.data_as(F64P),
                                             None, None, None, 0, 0, 0.0) == -1
    assert L.dh_last_error().decode() == "dh_reproject_surface_background: view row: malformed (finite members, scale positive, has-pivot flag 0 or 1)"
