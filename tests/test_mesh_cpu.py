"""Marching-cubes tables, the numpy restatement of the GPU mesh, PLY output and the density kernel's static checks
(no GPU needed)."""
import importlib.util
import os
import shutil
import sys

import numpy as np
import pytest

import mesh_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = M.tables


def face_of(e1, e2):
    """the cube face both edges lie on"""
    common = [f for f in range(6) if e1 in T.face_edges(f) and e2 in T.face_edges(f)]
    assert len(common) == 1, (e1, e2)
    return common[0]


def boundary(tris):
    """directed edges of a triangle set that have no reverse partner (the fan's diagonals cancel)"""
    d = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    return sorted(x for x in d if (x[1], x[0]) not in d)


def test_tables_reference_exactly_the_crossing_edges():
    counts, tris = T.build_tables()
    assert len(counts) == 256 and counts[0] == counts[255] == 0
    for case in range(256):
        used = sorted({e for t in tris[case] for e in t})
        assert used == T.crossing_edges(case), case
        assert all(len(set(t)) == 3 for t in tris[case])


def test_face_segments_depend_on_the_face_alone():
    # every case's triangle boundary, split by cube face, is a function of that face's four corner bits
    _, tris = T.build_tables()
    seen = {}
    for case in range(256):
        per_face = {f: [] for f in range(6)}
        for a, b in boundary(tris[case]):
            per_face[face_of(a, b)].append((a, b))
        for f in range(6):
            key = (f, tuple((case >> c) & 1 for c in T.face_walk(f)))
            segs = sorted(per_face[f])
            assert seen.setdefault(key, segs) == segs, (case, f)
    assert len(seen) == 6 * 16


def test_triangle_boundary_is_the_face_segments():
    _, tris = T.build_tables()
    for case in range(256):
        segs = sorted(s for f in range(6) for s in T.face_segments(f, T.case_inside(case)))
        assert boundary(tris[case]) == segs, case
        # each crossing edge starts one segment and ends another
        assert sorted(a for a, _ in segs) == sorted(b for _, b in segs) == T.crossing_edges(case)


def test_ambiguous_faces_separate_the_inside_corners():
    f = 0
    w = T.face_walk(f)
    case = (1 << w[0]) | (1 << w[2])
    segs = T.face_segments(f, T.case_inside(case))
    assert len(segs) == 2
    for a, b in segs:                          # each segment cuts off one inside corner: both edges touch it
        ca, cb = set(T.edge_corners(a)), set(T.edge_corners(b))
        assert len(ca & cb) == 1 and (ca & cb) <= {w[0], w[2]}


def test_header_is_current():
    want = T.render()
    assert open(os.path.join(ROOT, "nerf-simple_amd", "csrc", "mc_tables.h")).read() == want


@pytest.mark.parametrize("R", [(64, 64, 64), (97, 80, 71)])
def test_sphere_restatement(R):
    field, step = M.sphere_field(R)
    v, f, n = M.marching_cubes(field, 0.0, np.full(3, -1.0, np.float32), step)
    assert M.directed_edges_closed(f)
    assert M.euler_characteristic(v, f) == 2
    area, vol = M.area_and_volume(v, f)
    r = 0.6
    assert abs(area / (4 * np.pi * r * r) - 1) < 0.01
    assert vol > 0 and abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.01
    # normals point outward (along the radius, for a sphere)
    assert (np.einsum("ij,ij->i", n, v / np.linalg.norm(v, axis=1, keepdims=True)) > 0.99).all()


def test_torus_restatement():
    field, step = M.torus_field((72, 64, 56))
    v, f, _ = M.marching_cubes(field, 0.0, np.full(3, -1.0, np.float32), step)
    assert M.directed_edges_closed(f)
    assert M.euler_characteristic(v, f) == 0


def test_restatement_order_and_non_finite():
    # single cell, corner 0 inside: three vertices on its x, y, z edges (in that order), one outward triangle
    cell = np.zeros((2, 2, 2), np.float32)
    cell[0, 0, 0] = 1.0
    v, f, n = M.marching_cubes(cell, 0.5, np.zeros(3, np.float32), [np.float32(1)] * 3)
    assert np.array_equal(v, np.array([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]], np.float32))
    assert f.tolist() == [[0, 1, 2]]
    assert np.cross(v[1] - v[0], v[2] - v[0]) @ np.ones(3) > 0        # facing away from the inside corner
    # a non-finite corner: its cell emits nothing, its edges carry no vertex
    cell[1, 1, 1] = np.nan
    v, f, n = M.marching_cubes(cell, 0.5, np.zeros(3, np.float32), [np.float32(1)] * 3)
    assert v.shape == (3, 3) and f.shape == (0, 3)


def test_save_ply_round_trip(tmp_path):
    from nerf_simple_amd.utils import mesh
    field, step = M.sphere_field((16, 16, 16))
    v, f, n = M.marching_cubes(field, 0.0, np.full(3, -1.0, np.float32), step)
    rgb = np.random.default_rng(0).random((v.shape[0], 3)).astype(np.float32)
    path = mesh.save_ply(str(tmp_path / "s.ply"), v, f, n, rgb)
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert header[:2] == ["ply", "format binary_little_endian 1.0"]
    assert f"element vertex {v.shape[0]}" in header and f"element face {f.shape[0]}" in header
    props = [h.split()[-1] for h in header if h.startswith("property") and "list" not in h]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    vt = np.dtype([(p, "<f4") for p in props[:6]] + [(p, "u1") for p in props[6:]])
    body = np.frombuffer(data, dtype=vt, count=v.shape[0], offset=end)
    assert np.array_equal(np.stack([body["x"], body["y"], body["z"]], 1), v)
    assert np.array_equal(np.stack([body["nx"], body["ny"], body["nz"]], 1), n)
    assert np.array_equal(np.stack([body["red"], body["green"], body["blue"]], 1), np.rint(rgb * 255).astype(np.uint8))
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    faces = np.frombuffer(data, dtype=ft, offset=end + vt.itemsize * v.shape[0])
    assert (faces["n"] == 3).all() and np.array_equal(faces["v"], f)
    # without normals and colours
    path = mesh.save_ply(str(tmp_path / "b.ply"), v, f)
    assert b"property float nx" not in open(path, "rb").read(400)


def test_density_kernel_static_checks():
    """csrc/density.hip: 1936 MFMAs per kernel (layers 0..7 + the sigma tile), and its counted waits match the ISA."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_vmcnt
    finally:
        sys.path.pop(0)
    src = os.path.join(ROOT, "nerf-simple_amd", "csrc", "density.hip")
    for extra in ((), ("-DNERF_HALF",)):
        asm = check_vmcnt.assemble(src, extra)
        kernels = {k: v for k, v in check_vmcnt.kernels_of(asm).items() if "density" in k}
        assert len(kernels) == 2, list(kernels)
        for name, body in kernels.items():
            n, bad = check_vmcnt.check_kernel(body)
            assert n >= 30 and not bad, (name, n, bad)
            assert sum(1 for l in body if "v_mfma" in l) == 1936, name
