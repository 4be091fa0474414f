"""What the surface-mesh tests share (tests/test_meshes_host.py, tests/test_hip_meshes.py): an oracle that uses no route of
utilities/meshes.py - plain Python loops over cells and edges, straight from the definitions - the invariant checkers (closed,
Euler characteristic, the integer volume of a blocky mesh), small readers of the PLY and STL files, and the volumes the tests mesh.
Every volume is built once and never written to."""
import functools
import itertools
import json
import struct
from pathlib import Path

import numpy as np

import components_cases as cc

GOLDEN = Path(__file__).resolve().parent / "golden"
STYLES = ("smooth", "blocky")
DEGENERATE_SHAPES = [(1, 1, 1), (1, 1, 70), (1, 5, 1), (5, 1, 1), (2, 2, 2)]
CYCLIC = {2: (2, 1, 0), 1: (1, 0, 2), 0: (0, 2, 1)}      # axis a (0 = z, 1 = y, 2 = x) -> (a, b, c), the rotation of (x, y, z) that starts at a
AXIS_RANK = {0: 0, 1: 1, 2: 2}                           # within an owner: z, then y, then x


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def oracle_mesh(vol, value, style):
    """(vertices (V, 3) float32, quads (Q, 4) int32, quads per axis [z, y, x]) by the definitions, cell by cell and edge by edge"""
    vol = np.asarray(vol)
    extent = vol.shape
    grid = vol.tolist()

    def inside(p):
        return all(0 <= p[a] < extent[a] for a in range(3)) and grid[p[0]][p[1]][p[2]] == value

    def cell_index(cell):
        return (cell[0] * (extent[1] + 1) + cell[1]) * (extent[2] + 1) + cell[2]

    offsets = list(itertools.product((0, 1), repeat=3))
    cell_edges = [(p, q) for p in offsets for q in offsets if p < q and sum(abs(p[a] - q[a]) for a in range(3)) == 1]
    assert len(cell_edges) == 12
    ids, vertices = {}, []
    for cell in itertools.product(range(extent[0] + 1), range(extent[1] + 1), range(extent[2] + 1)):      # ascending cell index
        base = tuple(c - 1 for c in cell)
        corner = {d: inside(tuple(base[a] + d[a] for a in range(3))) for d in offsets}
        if len(set(corner.values())) == 1:
            continue
        ids[cell] = len(vertices)
        if style == "blocky":
            off = [np.float32(0.5)] * 3
        else:
            crossing = [(p, q) for p, q in cell_edges if corner[p] != corner[q]]
            n = len(crossing)
            assert 1 <= n <= 12
            off = [np.float32(np.float64(sum(p[a] + q[a] for p, q in crossing)) / np.float64(2 * n)) for a in range(3)]      # twice a midpoint = the sum of its two corners
        vertices.append([np.float32(base[a]) + off[a] for a in range(3)])

    found = []
    per_axis = [0, 0, 0]
    for a in range(3):
        _, b, c = CYCLIC[a]
        ranges = [range(extent[0]), range(extent[1]), range(extent[2])]
        ranges[a] = range(-1, extent[a])                              # the lower position; outside the volume on the first and beyond it on the last
        for low in itertools.product(*ranges):
            high = tuple(low[t] + (t == a) for t in range(3))
            if inside(low) == inside(high):
                continue
            around = []
            for db, dc in itertools.product((0, 1), repeat=2):        # the four cells that have both positions as corners
                cell = [0, 0, 0]
                cell[a], cell[b], cell[c] = low[a] + 1, low[b] + db, low[c] + dc
                around.append(tuple(cell))
            owner = max(around, key=cell_index)
            order = [(-1, -1), (0, -1), (0, 0), (-1, 0)] if inside(low) else [(-1, -1), (-1, 0), (0, 0), (0, -1)]
            quad = []
            for db, dc in order:
                cell = list(owner)
                cell[b] += db
                cell[c] += dc
                quad.append(ids[tuple(cell)])
            found.append((cell_index(owner), AXIS_RANK[a], quad))
            per_axis[a] += 1
    found.sort(key=lambda f: (f[0], f[1]))
    return (np.array(vertices, dtype=np.float32).reshape(-1, 3), np.array([f[2] for f in found], dtype=np.int32).reshape(-1, 4), per_axis)


@functools.lru_cache(maxsize=None)
def oracle_cached(name, value, style):
    """the oracle of a named volume of VOLUMES, computed once and shared"""
    v, q, per_axis = oracle_mesh(VOLUMES[name](), value, style)
    v.setflags(write=False)
    q.setflags(write=False)
    return v, q, tuple(per_axis)


def assert_mesh_equal(got, want, what=""):
    """`got`: the dict of extract_surface or (vertices, quads, per axis); `want`: the oracle's triple.  Bit for bit."""
    gv, gq, ga = (got["vertices"], got["quads"], got["quads_per_axis"]) if isinstance(got, dict) else got
    wv, wq, wa = (want["vertices"], want["quads"], want["quads_per_axis"]) if isinstance(want, dict) else want
    assert [int(x) for x in ga] == [int(x) for x in wa], (what, list(ga), list(wa))
    assert gv.shape == wv.shape and gv.dtype == np.float32 and wv.dtype == np.float32, (what, gv.shape, wv.shape, gv.dtype)
    assert gq.shape == wq.shape and gq.dtype == np.int32, (what, gq.shape, wq.shape, gq.dtype)
    assert gv.tobytes() == wv.tobytes(), (what, np.argwhere(gv != wv)[:6].tolist(), gv[gv != wv][:6], wv[gv != wv][:6])
    assert np.array_equal(gq, wq), (what, np.argwhere(gq != wq)[:6].tolist(), gq[gq != wq][:6], wq[gq != wq][:6])


# ---- invariants ------------------------------------------------------------------------------------------------------------------
def directed_edges(quads):
    count = {}
    for q in np.asarray(quads).tolist():
        for t in range(4):
            e = (q[t], q[(t + 1) % 4])
            count[e] = count.get(e, 0) + 1
    return count


def is_closed(quads):
    count = directed_edges(quads)
    return all(count.get((v, u), 0) == n for (u, v), n in count.items())


def quads_per_edge(quads):
    """{undirected edge: quads that use it}"""
    uses = {}
    for (u, v), n in directed_edges(quads).items():
        key = (min(u, v), max(u, v))
        uses[key] = uses.get(key, 0) + n
    return uses


def euler_characteristic(vertices, quads):
    return len(vertices) - len(quads_per_edge(quads)) + len(quads)


def volume_times_48(vertices, quads):
    """the sum over the triangles of det(P0, P1, P2) with P = twice the position read as (x, y, z), in Python integers: 8 x 6 x the
    enclosed volume for positions that are multiples of one half - a blocky mesh's - and positive for the outward winding"""
    twice = [[int(round(2 * float(c))) for c in (p[2], p[1], p[0])] for p in np.asarray(vertices).tolist()]
    assert all(abs(2 * float(c) - round(2 * float(c))) == 0 for p in np.asarray(vertices).tolist() for c in p)
    total = 0
    for q in np.asarray(quads).tolist():
        for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
            a, b, c = (twice[t] for t in tri)
            total += (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))
    return total


def check_invariants(vol, value, vertices, quads, per_axis, blocky):
    assert is_closed(quads)
    assert len(quads) == sum(per_axis)
    if blocky:
        assert volume_times_48(vertices, quads) == 48 * int((np.asarray(vol) == value).sum())


# ---- file readers ----------------------------------------------------------------------------------------------------------------
def read_ply(path):
    """(header lines, vertices (V, 3) float32 as x y z, faces as a list of index lists, file size)"""
    data = Path(path).read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n_vertices = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    n_faces = int(next(l for l in lines if l.startswith("element face")).split()[-1])
    vertices = np.frombuffer(data, dtype="<f4", count=3 * n_vertices, offset=end).reshape(-1, 3)
    at, faces = end + 12 * n_vertices, []
    for _ in range(n_faces):
        corners = data[at]
        faces.append(list(struct.unpack_from(f"<{corners}i", data, at + 1)))
        at += 1 + 4 * corners
    assert at == len(data)
    return lines, vertices, faces, len(data)


def read_stl(path):
    """(triangle count, records as (T, 12) float32: normal, a, b, c; file size)"""
    data = Path(path).read_bytes()
    count = struct.unpack_from("<I", data, 80)[0]
    assert len(data) == 84 + 50 * count
    records = np.array([struct.unpack_from("<12f", data, 84 + 50 * t) for t in range(count)], dtype=np.float32).reshape(-1, 12)
    assert all(struct.unpack_from("<H", data, 84 + 50 * t + 48)[0] == 0 for t in range(count))
    return count, records, len(data)


# ---- volumes ---------------------------------------------------------------------------------------------------------------------
def frozen(vol):
    vol = np.ascontiguousarray(vol, dtype=np.uint8)
    vol.setflags(write=False)
    return vol


def one_voxel():
    return frozen(np.ones((1, 1, 1)))


def solid_box(shape=(4, 5, 6)):
    """a box of value 1 with one voxel of 0 around it"""
    vol = np.zeros(tuple(s + 2 for s in shape), dtype=np.uint8)
    vol[1:-1, 1:-1, 1:-1] = 1
    return frozen(vol)


def box_with_through_hole():
    vol = np.array(solid_box((5, 5, 4)))
    vol[:, 3, 2:4] = 0                                                # a tunnel along z, open at both ends
    return frozen(vol)


def hollow_shell():
    """value 2 of cc.shells: one closed shell with an inside and an outside surface (depth 1 of 0 .. 2 in a 7 x 7 x 8 volume)"""
    return frozen(cc.shells((7, 7, 8)))


def edge_pair():
    return frozen(cc.pair_touching("edge_yx", (2, 2, 3), shape=(4, 4, 6)))


def row_runs(x):
    """(3, 4, x) random labels 0 / 1 with a run of 1 along a whole row and one that stops 3 cells short of the row's end"""
    vol = np.array(cc.random_labels((3, 4, x), 2, 0.5, x))
    vol[0, 1, :] = 1
    vol[1, 2, :] = 0
    vol[1, 2, 5:x - 3] = 1
    return frozen(vol)


def touching_every_face():
    vol = np.zeros((5, 6, 70), dtype=np.uint8)
    vol[:, 2:4, 10:60] = 1
    vol[2, :, 30:33] = 1
    vol[1:3, 2, :] = 1
    return frozen(vol)


VOLUMES = {
    "one_voxel": one_voxel,
    "solid_box": solid_box,
    "through_hole": box_with_through_hole,
    "shell": hollow_shell,
    "edge_pair": edge_pair,
    "checkerboard": lambda: frozen(cc.checkerboard((4, 5, 9))),
    "random_k2": lambda: frozen(cc.random_labels((5, 6, 7), 2, 0.5, 11)),
    "random_k4": lambda: frozen(cc.random_labels((6, 5, 9), 4, 0.6, 12)),
    "every_face": touching_every_face,
}
VOLUMES.update({f"degenerate_{'x'.join(map(str, s))}": (lambda s=s: frozen(cc.random_labels(s, 2, 0.6, sum(s)))) for s in DEGENERATE_SHAPES})


@functools.lru_cache(maxsize=None)
def vessels_expected():
    return json.loads((GOLDEN / "mesh_vessels.json").read_text())


def write_vessels_golden():
    """tests/golden/mesh_vessels.json from the host route: per non-zero value and style the vertices, the quads per axis and the digest"""
    from volume_segmantics_amd.utilities import meshes
    vol, doc = cc.vessels(), {}
    for value in [v for v in np.unique(vol).tolist() if v != 0]:
        doc[str(value)] = {}
        for style in STYLES:
            s = meshes.extract_surface(vol, value, style, device="cpu")
            doc[str(value)][style] = {"vertices": len(s["vertices"]), "quads_per_axis": s["quads_per_axis"].tolist(), "sha256": digest(s)}
    (GOLDEN / "mesh_vessels.json").write_text(json.dumps(doc, indent=1) + "\n")


def digest(surface):
    """SHA-256 over the vertex bytes then the quad bytes"""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(surface["vertices"]).tobytes() + np.ascontiguousarray(surface["quads"]).tobytes()).hexdigest()
