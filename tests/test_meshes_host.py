"""The host side of utilities/meshes.py (no GPU): the host route bit for bit against the cell-by-cell oracle of tests/mesh_cases.py in
both styles, the one-voxel closed forms, the invariants (closed, the exact integer volume of a blocky mesh whose sign pins the
winding, Euler characteristics, the 4-quad edge), the quads per axis against the exposed faces that ``measure`` counts, the PLY and
STL writers read back, the settings keys and error cases, the mesh command, and the committed vessels figures.  Nothing has a
tolerance."""
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import components_cases as cc
import measurement_cases as measured
import mesh_cases as mc
from volume_segmantics_amd.utilities import measurements
from volume_segmantics_amd.utilities import meshes as me

REPO = Path(__file__).resolve().parent.parent


def host(vol, value, style="smooth"):
    return me.extract_surface(vol, value, style, device="cpu")


# ---- the arrays ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", mc.STYLES)
@pytest.mark.parametrize("name", sorted(mc.VOLUMES))
def test_host_route_against_the_oracle(name, style):
    vol = mc.VOLUMES[name]()
    for value in sorted(set(np.unique(vol).tolist()) | {0, 9}):      # 9 occurs nowhere; 0 meshes the background
        want = mc.oracle_cached(name, value, style)
        got = host(vol, value, style)
        mc.assert_mesh_equal(got, want, (name, value, style))
        assert got["shape"].tolist() == list(vol.shape)
        mc.check_invariants(vol, value, got["vertices"], got["quads"], got["quads_per_axis"], style == "blocky")
        assert me.mesh_summary(got)["closed"] is True


def test_one_voxel():
    smooth, blocky = host(mc.one_voxel(), 1), host(mc.one_voxel(), 1, "blocky")
    for s in (smooth, blocky):
        assert s["vertices"].shape == (8, 3) and s["quads"].shape == (6, 4) and s["quads_per_axis"].tolist() == [2, 2, 2]
        assert sorted(s["quads"].reshape(-1).tolist()) == sorted(list(range(8)) * 3)
    sixth = np.float32(np.float64(1) / np.float64(6))                 # an offset of 1/6 from the voxel centre: a cube of side 1/3
    low = np.float32(-1) + np.float32(np.float64(5) / np.float64(6))
    assert sorted(set(smooth["vertices"].reshape(-1).tolist())) == [float(low), float(sixth)]
    assert sorted(set(blocky["vertices"].reshape(-1).tolist())) == [-0.5, 0.5]
    a, b = me.mesh_summary(smooth), me.mesh_summary(blocky)
    assert (b["surface_area"], b["enclosed_volume"], b["euler_characteristic"], b["triangles"]) == (6.0, 1.0, 2, 12)
    assert b["bounding_box"] == [[-0.5] * 3, [0.5] * 3]
    side = float(sixth) - float(low)
    assert a["surface_area"] == pytest.approx(6 * side * side, rel=1e-12) and a["enclosed_volume"] == pytest.approx(side ** 3, rel=1e-12)
    scaled = me.mesh_summary(blocky, [3.0, 2.0, 1.0])
    assert scaled["enclosed_volume"] == 6.0 and scaled["surface_area"] == 2 * (6.0 + 3.0 + 2.0) and scaled["bounding_box"][1] == [1.5, 1.0, 0.5]


def test_euler_characteristics_and_the_non_manifold_edge():
    for name, value, euler in (("solid_box", 1, 2), ("through_hole", 1, 0), ("shell", 2, 4)):
        for style in mc.STYLES:
            s = host(mc.VOLUMES[name](), value, style)
            assert mc.euler_characteristic(s["vertices"], s["quads"]) == euler, (name, style)
            figures = me.mesh_summary(s)
            assert figures["euler_characteristic"] == euler and figures["closed"] and figures["non_manifold_edges"] == 0
    pair = host(mc.edge_pair(), 1, "blocky")
    uses = mc.quads_per_edge(pair["quads"])
    assert sorted(uses.values())[-2:] == [2, 4] and mc.is_closed(pair["quads"])       # one edge carries 4 quads and the mesh is still closed
    assert len(pair["vertices"]) == 14 and me.mesh_summary(pair)["non_manifold_edges"] == 1
    assert mc.volume_times_48(pair["vertices"], pair["quads"]) == 48 * 2


def test_winding_is_outward():
    """a blocky box: the integer volume is positive, and every triangle's normal points away from the box's centre"""
    vol = mc.solid_box()
    s = host(vol, 1, "blocky")
    assert mc.volume_times_48(s["vertices"], s["quads"]) == 48 * int((vol == 1).sum())
    p = s["vertices"][:, ::-1].astype(np.float64)                     # (x, y, z)
    tri = me.triangles_of(s["quads"])
    normal = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    outward = (p[tri[:, 0]] + p[tri[:, 1]] + p[tri[:, 2]]) / 3 - p.mean(axis=0)
    assert ((normal * outward).sum(axis=1) > 0).all()
    inverse = host(vol, 0, "blocky")                                  # the background's surface: the box's, wound the other way, and the volume's boundary
    assert mc.volume_times_48(inverse["vertices"], inverse["quads"]) == 48 * int((vol == 0).sum())


@pytest.mark.parametrize("name", ["random_k4", "checkerboard", "every_face", "degenerate_2x2x2", "shell"])
def test_quads_per_axis_are_the_exposed_faces_of_measure(name):
    vol = mc.VOLUMES[name]()
    assert min(vol.shape) >= 2
    raw = measurements.measure_components(vol, include_background=True, device="cpu")
    for value in np.unique(vol).tolist():
        rows = raw["table"][raw["values"] == value]
        faces = [int(rows[:, measurements.F["faces_" + axis]].sum()) for axis in "zyx"]
        assert host(vol, value)["quads_per_axis"].tolist() == faces, (name, value)


# ---- the files -------------------------------------------------------------------------------------------------------------------
def test_ply_and_stl_read_back(tmp_path):
    vol = mc.VOLUMES["random_k4"]()
    s = host(vol, 2)
    size = [2.0, 1.0, 0.5]
    xyz = (s["vertices"].astype(np.float64)[:, ::-1] * np.array(size[::-1])).astype(np.float32)
    n_vertices, n_quads = len(s["vertices"]), len(s["quads"])
    assert n_quads > 20

    lines, vertices, faces, nbytes = mc.read_ply(me.write_ply(tmp_path / "q.ply", s, size))
    assert f"element vertex {n_vertices}" in lines and f"element face {n_quads}" in lines and lines[-1] == "end_header"
    assert [l for l in lines if l.startswith("property")] == ["property float x", "property float y", "property float z", "property list uchar int vertex_indices"]
    assert vertices.tobytes() == xyz.tobytes()
    assert faces[0] == s["quads"][0].tolist() and faces[-1] == s["quads"][-1].tolist() and len(faces) == n_quads
    assert nbytes == len("\n".join(lines)) + 1 + 12 * n_vertices + 17 * n_quads

    lines, vertices, faces, nbytes = mc.read_ply(me.write_ply(tmp_path / "t.ply", s, size, triangulate=True))
    q0, q1 = s["quads"][0].tolist(), s["quads"][-1].tolist()
    assert f"element face {2 * n_quads}" in lines and faces[0] == q0[:3] and faces[1] == [q0[0], q0[2], q0[3]] and faces[-1] == [q1[0], q1[2], q1[3]]
    assert nbytes == len("\n".join(lines)) + 1 + 12 * n_vertices + 13 * 2 * n_quads

    count, records, nbytes = mc.read_stl(me.write_stl(tmp_path / "t.stl", s, size))
    assert count == 2 * n_quads and nbytes == 84 + 50 * count
    assert records[0, 3:].tobytes() == xyz[q0[:3]].tobytes() and records[-1, 3:].tobytes() == xyz[[q1[0], q1[2], q1[3]]].tobytes()
    a, b, c = (records[:, 3 + 3 * t:6 + 3 * t].astype(np.float64) for t in range(3))
    normal = np.cross(b - a, c - a)
    length = np.linalg.norm(normal, axis=1)
    assert np.allclose(records[length > 0, :3], (normal / np.maximum(length, 1e-300)[:, None])[length > 0], atol=1e-5)     # the stored normal is the winding's
    assert (records[length == 0, :3] == 0).all()

    empty = host(vol, 9)
    assert mc.read_ply(me.write_ply(tmp_path / "e.ply", empty))[3] == len((tmp_path / "e.ply").read_bytes()) and mc.read_stl(me.write_stl(tmp_path / "e.stl", empty))[0] == 0


def test_write_meshes_and_summary(tmp_path):
    vol = mc.VOLUMES["random_k4"]()
    m = me.mesh_label_volume(vol, SimpleNamespace(mesh_format="stl", mesh_voxel_size=[2.0, 1.0, 1.0], mesh_style="blocky"), device="cpu")
    assert list(m["surfaces"]) == [1, 2, 3] and list(m["summary"]) == ["1", "2", "3"] and m["shape"] == list(vol.shape)
    written = me.write_meshes(tmp_path / "seg", m)
    assert [p.name for p in written] == ["seg_mesh_1.stl", "seg_mesh_2.stl", "seg_mesh_3.stl", "seg_meshes.json"]
    doc = json.loads(written[-1].read_text())
    assert doc["settings"] == m["settings"] and doc["shape"] == list(vol.shape)
    for value in (1, 2, 3):
        row = doc["meshes"][str(value)]
        assert row["file"] == f"seg_mesh_{value}.stl" and {k: v for k, v in row.items() if k != "file"} == m["summary"][str(value)]
        assert row["enclosed_volume"] == 2.0 * int((vol == value).sum()) and row["closed"] is True
        assert mc.read_stl(tmp_path / row["file"])[0] == row["triangles"]
    assert me.mesh_summary_text(m["summary"]).count("\n") == 3


# ---- settings, errors, command -----------------------------------------------------------------------------------------------------
def test_settings_defaults_and_parsing():
    assert me.mesh_settings(SimpleNamespace()) == dict(active=False, values=None, style="smooth", format="ply", triangulate=False, voxel_size=[1.0, 1.0, 1.0])
    on = me.mesh_settings(SimpleNamespace(mesh_surfaces=True, mesh_values=[3, 1, 3], mesh_style="blocky", mesh_format="stl", mesh_triangulate=True,
                                          mesh_voxel_size=[2, 0.5, 1]))
    assert on == dict(active=True, values=[1, 3], style="blocky", format="stl", triangulate=True, voxel_size=[2.0, 0.5, 1.0])
    assert me.mesh_settings(SimpleNamespace(measure_voxel_size=0.25))["voxel_size"] == [0.25] * 3
    assert me.mesh_settings(SimpleNamespace(measure_voxel_size=0.25, mesh_voxel_size=2))["voxel_size"] == [2.0] * 3
    assert me.mesh_settings(SimpleNamespace(mesh_values=7))["values"] == [7]
    for bad in (dict(mesh_style="marching"), dict(mesh_format="obj"), dict(mesh_voxel_size=[1, 2]), dict(mesh_voxel_size=0), dict(mesh_values=[1, 256])):
        with pytest.raises(ValueError):
            me.mesh_settings(SimpleNamespace(**bad))
    shipped = (REPO / "volseg-settings" / "2d_model_predict_settings.yaml").read_text()
    for key in ("mesh_surfaces", "mesh_values", "mesh_style", "mesh_format", "mesh_triangulate", "mesh_voxel_size"):
        assert f"# {key}:" in shipped                                # documented, commented out: the shipped settings mesh nothing
    from volume_segmantics_amd.data import get_settings_data
    assert not me.mesh_settings(get_settings_data(REPO / "volseg-settings" / "2d_model_predict_settings.yaml"))["active"]


def test_error_cases():
    vol = mc.VOLUMES["random_k2"]()
    with pytest.raises(ValueError, match="style"):
        host(vol, 1, "marching")
    with pytest.raises(ValueError, match="uint8"):
        host(vol, 256)
    for shape in ((1289, 1289, 1290), (1 << 30, 1, 1)):               # decided from the extents alone: nothing of that size is touched
        huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=shape, strides=(0, 0, 0))
        with pytest.raises(ValueError, match="2\\^31"):
            me.extract_surface(huge, 1, device="cpu")
    with pytest.raises(TypeError):
        host(vol.astype(np.float32), 1)


def test_manager_keys_absent_and_one_hot(tmp_path, monkeypatch):
    """without the keys the manager's meshing branch is not entered and no mesh file appears; with them the files are written; one_hot
    with mesh_surfaces is refused"""
    from volume_segmantics_amd.model.operations import vol_seg_prediction_manager as pm
    labels = mc.VOLUMES["random_k4"]()
    fake = SimpleNamespace(_predict_single_axis=lambda vol, axis: (labels, None), model_device_num=0)
    settings = SimpleNamespace(one_hot=False, quality="low", prediction_axis="Z", output_probs=False)
    manager = pm.VolSeg2DPredictionManager.__new__(pm.VolSeg2DPredictionManager)
    manager.predictor, manager.settings, manager.data_vol, manager.input_data_chunking = fake, settings, labels, True
    real = me.mesh_label_volume
    monkeypatch.setattr(me, "mesh_label_volume", lambda *a, **k: pytest.fail("meshed without the key"))
    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    manager.predict_volume_to_path(tmp_path / "off" / "seg.h5")
    settings.mesh_surfaces = False
    manager.predict_volume_to_path(tmp_path / "off" / "seg.h5")
    assert manager.last_meshes is None and [p.name for p in (tmp_path / "off").iterdir()] == ["seg.h5"]
    monkeypatch.setattr(me, "mesh_label_volume", lambda vol, s, device=None: real(vol, s, device="cpu"))
    settings.mesh_surfaces, settings.mesh_values = True, [2]
    manager.predict_volume_to_path(tmp_path / "on" / "seg.h5")
    assert sorted(p.name for p in (tmp_path / "on").iterdir()) == ["seg.h5", "seg_mesh_2.ply", "seg_meshes.json"]
    assert (tmp_path / "on" / "seg.h5").read_bytes() == (tmp_path / "off" / "seg.h5").read_bytes()
    mc.assert_mesh_equal(manager.last_meshes["surfaces"][2], mc.oracle_cached("random_k4", 2, "smooth"))
    settings.one_hot = True
    with pytest.raises(ValueError, match="one_hot"):
        manager.predict_volume_to_path(None)


def test_mesh_command_on_an_hdf5_file(tmp_path):
    """the file is written and read through base_data_utils; the command meshes on a host without a GPU and without mesh_surfaces"""
    from volume_segmantics_amd.scripts import mesh_2d_prediction
    from volume_segmantics_amd.utilities import arg_parsing
    from volume_segmantics_amd.utilities import base_data_utils as utils
    vol = np.array([0, 7, 100, 200], dtype=np.uint8)[mc.VOLUMES["random_k4"]()]
    (tmp_path / "volseg-settings").mkdir()
    (tmp_path / "volseg-settings" / "2d_model_predict_settings.yaml").write_text("mesh_values: [7, 200]\nmesh_style: blocky\nmeasure_voxel_size: [2.0, 1.0, 1.0]\n")
    utils.save_data_to_hdf5(vol, tmp_path / "pred.h5")
    mesh_2d_prediction.main([str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path)])
    assert {p.name for p in tmp_path.iterdir()} == {"volseg-settings", "pred.h5", "pred_mesh_7.ply", "pred_mesh_200.ply", "pred_meshes.json"}
    doc = json.loads((tmp_path / "pred_meshes.json").read_text())
    assert doc["settings"]["voxel_size"] == [2.0, 1.0, 1.0] and doc["settings"]["style"] == "blocky" and list(doc["meshes"]) == ["7", "200"]
    want = mc.oracle_cached("random_k4", 1, "blocky")                 # value 7 is value 1 of the volume before the lookup
    lines, vertices, faces, _ = mc.read_ply(tmp_path / "pred_mesh_7.ply")
    assert f"element vertex {len(want[0])}" in lines and f"element face {len(want[1])}" in lines
    assert faces == want[1].tolist() and vertices.tobytes() == (want[0].astype(np.float64)[:, ::-1] * np.array([1.0, 1.0, 2.0])).astype(np.float32).tobytes()
    assert doc["meshes"]["7"]["enclosed_volume"] == 2.0 * int((vol == 7).sum())
    mesh_2d_prediction.main([str(tmp_path / "pred.h5"), "--data_dir", str(tmp_path), "--output", str(tmp_path / "other")])
    assert (tmp_path / "other_mesh_200.ply").read_bytes() == (tmp_path / "pred_mesh_200.ply").read_bytes()
    for bad in ([str(tmp_path / "missing.h5")], [str(tmp_path / "pred.h5"), "--output", str(tmp_path / "nowhere" / "stem")], []):
        with pytest.raises(SystemExit) as stop:
            arg_parsing.parse_meshing_args(bad)
        assert stop.value.code == 2


# ---- the vessels fixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", mc.STYLES)
def test_vessels_fixture_against_the_committed_figures(style):
    """tests/golden/mesh_vessels.json holds per non-zero value and style the vertices, the quads per axis and a SHA-256 of the vertex
    and quad bytes, written once by the host route:

        python -c "import sys; sys.path.insert(0, 'tests'); import mesh_cases; mesh_cases.write_vessels_golden()"
    """
    vol = cc.vessels()
    expected = mc.vessels_expected()
    assert sorted(expected) == [str(v) for v in np.unique(vol).tolist() if v != 0]
    table = measured.vessels_expected()["6"]
    for value, per_style in expected.items():
        s = host(vol, int(value), style)
        want = per_style[style]
        assert len(s["vertices"]) == want["vertices"] and s["quads_per_axis"].tolist() == want["quads_per_axis"] and mc.digest(s) == want["sha256"]
        rows = [row for row, v in zip(table["table"], table["values"]) if v == int(value)]      # the committed integers of measure, background included
        assert want["quads_per_axis"] == [sum(row[measurements.F["faces_" + axis]] for row in rows) for axis in "zyx"]
