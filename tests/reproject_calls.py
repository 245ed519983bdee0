"""What decides which re-projection call a plan is: the members of depth_transform.reproject_record(p, K) that used to pick a
positional entry and its workspace query by name.  `fields(p)` reads them off the record; the constants are the values each of
those names stood for (the plan's former rule: a camera; else the table, with or without a donor; else the identity table; then
border, surfaces and bones on top -- and border and surfaces for the kinds without a foreground point)."""
from diffusionhandles_amd import depth_transform as DT


def fields(p, K=None):
    r = DT.reproject_record(p, len(p.edits) if K is None else K)
    return dict(points=r.n_fg > 0, table=bool(r.inst_obj) and r.n_instances > 0, views=bool(r.has_view), donor=r.n_donor_objects > 0,
                border=r.infill_border, surfaces=r.view_surfaces, bones=r.n_bones)


# dh_reproject_footprint_edits on dh_reproject_footprints_workspace_bytes: the identity table on its own carving, nothing else
FOOTPRINT = dict(points=True, table=False, views=False, donor=False, border=0, surfaces=0, bones=0)
# dh_reproject_instance_edits on dh_reproject_instances_workspace_bytes
INSTANCE = dict(FOOTPRINT, table=True)
# dh_reproject_donor_edits (sized by the instance query)
DONOR = dict(INSTANCE, donor=True)
# dh_reproject_camera_edits on dh_reproject_camera_workspace_bytes
CAMERA = dict(INSTANCE, views=True)
# dh_reproject_surface_edits on dh_reproject_surface_ws_bytes
SURFACE = dict(CAMERA, surfaces=1)
# dh_reproject_background on dh_reproject_background_workspace_bytes, and dh_reproject_camera_background on the same
BACKGROUND = dict(points=False, table=False, views=False, donor=False, border=0, surfaces=0, bones=0)
CAMERA_BACKGROUND = dict(BACKGROUND, views=True)
# dh_reproject_surface_background on dh_reproject_surface_background_ws_bytes
SURFACE_BACKGROUND = dict(CAMERA_BACKGROUND, surfaces=1)


def border(call):
    """dh_reproject_border_edits / dh_reproject_border_background in place of `call`: the same members and the reflecting border
    (on the workspace of the call it extends; a call without a table gains it)"""
    return dict(call, border=1, table=call["table"] or call["points"])
