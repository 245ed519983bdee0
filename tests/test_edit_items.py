"""CPU: the batched planned-energy entries in the C ABI (header, ctypes table, exported symbols) and the packing of a
test set's edits into mixed-image batches (parallel.pack_edit_batches) on the reference's own test set."""
import json
import os
import re
from collections import OrderedDict

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("dh_energy_planned_batch_workspace_bytes", "dh_energy_fwd_bwd_planned_batch")


def _header_arity(name):
    txt = open(os.path.join(ROOT, "include", "diffhandles_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt, flags=re.S)
    assert m, f"{name} is not declared in include/diffhandles_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_batched_energy_entries_are_declared_bound_and_exported():
    from diffusionhandles_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.lib()
    for name in NEW_ENTRIES:
        n = _header_arity(name)
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert len(_lib.SIGNATURES[name][1]) == n, (name, len(_lib.SIGNATURES[name][1]), n)
        assert name not in lib.dh_missing_symbols and hasattr(lib, name), f"{name} is not exported by the built library"
    # the item structure of the header, field for field
    txt = open(os.path.join(ROOT, "include", "diffhandles_hip.h")).read()
    body = re.search(r"typedef struct dh_energy_item \{(.*?)\} dh_energy_item;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.split(r"[\s*]+", part.strip())[-1] for part in decl.split(",")]
    assert fields == [f for f, _ in _lib.EnergyItem._fields_], fields


def _photogen():
    with open(os.path.join(ROOT, "tests", "golden", "photogen", "photogen.json")) as f:
        return list(json.load(f, object_pairs_hook=OrderedDict).items())


def test_pack_edit_batches_on_the_photogen_test_set():
    from diffusionhandles_amd.parallel import pack_edit_batches
    scenes = _photogen()
    flat = [(s, n) for s, names in scenes for n in names]
    assert len(scenes) == 20 and len(flat) == 90 and len(set(flat)) == 90
    b8 = pack_edit_batches(scenes, 8)
    assert [len(b) for b in b8] == [8] * 11 + [2]
    assert [p for b in b8 for p in b] == flat                      # test-set order, every pair exactly once
    b1 = pack_edit_batches(scenes, 1)
    assert len(b1) == 90 and [b[0] for b in b1] == flat
    per_scene = pack_edit_batches(scenes, 8, max_images=1)
    assert len(per_scene) == 23 == sum(-(-len(names) // 8) for _, names in scenes)
    assert all(len({s for s, _ in b}) == 1 and len(b) <= 8 for b in per_scene)
    assert [p for b in per_scene for p in b] == flat
    two = pack_edit_batches(scenes, 8, max_images=2)
    assert max(len({s for s, _ in b}) for b in two) == 2 and all(len(b) <= 8 for b in two)
    assert [p for b in two for p in b] == flat
    # a scene's edits are contiguous inside every batch
    for b in b8 + two:
        names = [s for s, _ in b]
        seen = []
        for s in names:
            if not seen or seen[-1] != s:
                assert s not in seen
                seen.append(s)


def test_pack_edit_batches_edge_cases():
    from diffusionhandles_amd.parallel import pack_edit_batches
    assert pack_edit_batches([], 4) == []
    assert pack_edit_batches([("a", []), ("b", ["x"])], 4) == [[("b", "x")]]
    assert pack_edit_batches([("a", ["1", "2", "3"])], 2) == [[("a", "1"), ("a", "2")], [("a", "3")]]
    # a scene that runs over into the next batch counts as that batch's first image
    got = pack_edit_batches([("a", ["1", "2", "3"]), ("b", ["1"]), ("c", ["1"])], 2, max_images=2)
    assert got == [[("a", "1"), ("a", "2")], [("a", "3"), ("b", "1")], [("c", "1")]]
    with pytest.raises(ValueError):
        pack_edit_batches([("a", ["1"])], 0)
    with pytest.raises(ValueError):
        pack_edit_batches([("a", ["1"])], 2, max_images=0)
