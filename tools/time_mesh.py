"""Time the density grid and marching cubes on one GPU (profiles/mesh_timing.json).

  * sigma-only kernel (nerf_amd_density_grid, grid formed in the kernel) against the points-mode forward
    (nerf_amd_mlp_forward on a [P,6] table), per point, fp16 and bf16, at 256^3 and 512^3;
  * marching cubes at 512^3 on the sigma grid of a synthetic net: ms per pass and the bytes each pass moves;
  * the whole extraction (density grid + marching cubes) against the density pass alone.
Times are HIP events around back-to-back launches after a warm-up, median of the repeats.

usage: python tools/time_mesh.py [--out profiles/mesh_timing.json] [--reps 5]     (GPU box; one process, one device)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import nerf_simple_amd  # noqa: E402,F401
from nerf_simple_amd import _lib  # noqa: E402
from nerf_simple_amd.utils import mesh, synthetic  # noqa: E402
from nerf_simple_amd.utils.nets import Nerf  # noqa: E402

PEAK_FLOPS = 2.5e15                     # dense 16-bit MFMA peak the issue's fraction refers to
FLOP_PER_32_POINTS = 1936 * 16384       # sigma network: 1936 MFMAs of 16x16x32 (2 * 16 * 16 * 32 FLOP) per wave-tile
FLOP_PER_32_POINTS_FULL = 2344 * 16384


def timed(fn, reps, inner=1):
    """median ms per call of fn over `reps` event-timed groups of `inner` calls (after one warm-up group)"""
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return statistics.median(out)


def f3(a):
    return (ctypes.c_float * 3)(*[float(x) for x in a])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    st = _lib.stream_ptr(dev)
    res = {"device": torch.cuda.get_device_name(0), "density": [], "marching_cubes": {}}
    net = Nerf().to(dev)
    net.load_state_dict(synthetic.synthetic_state_dict(0, "structured"))
    bounds = ((-1.0,) * 3, (1.0,) * 3)
    for precision in ("fp16", "bf16"):
        code = _lib.precision_code(precision)
        packed = net.packed_weights(code)
        for r in (256, 512):
            R = (r, r, r)
            P = r ** 3
            lo, step = mesh.grid_axes(R, bounds)
            sigma = torch.empty(R, dtype=torch.float32, device=dev)
            pts = torch.empty((P, 6), dtype=torch.float32, device=dev)
            _lib.check(lib.nerf_amd_grid_points(f3(lo), f3(step), *R, 0, P, _lib.ptr(pts), st), "grid_points")
            out = torch.empty((P, 4), dtype=torch.float32, device=dev)
            t_d = timed(lambda: lib.nerf_amd_density_grid(f3(lo), f3(step), *R, _lib.ptr(packed), code, _lib.ptr(sigma), st),
                        args.reps)
            t_f = timed(lambda: lib.nerf_amd_mlp_forward(_lib.ptr(pts), _lib.ptr(packed), _lib.ptr(out), P, code, st), args.reps)
            sig_pts = torch.empty(P, dtype=torch.float32, device=dev)
            t_p = timed(lambda: lib.nerf_amd_density_forward(_lib.ptr(pts), 6, _lib.ptr(packed), code, _lib.ptr(sig_pts), P, st),
                        args.reps)
            torch.cuda.synchronize()
            same = bool(torch.equal(sigma.view(-1).view(torch.int32), out[:, 3].contiguous().view(torch.int32)))
            row = {
                "precision": precision, "grid": r, "points": P,
                "density_grid_ms": round(t_d, 3), "density_points_ms": round(t_p, 3), "forward_points_ms": round(t_f, 3),
                "ns_per_point_density": round(t_d * 1e6 / P, 4), "ns_per_point_forward": round(t_f * 1e6 / P, 4),
                "throughput_ratio_grid_vs_forward": round(t_f / t_d, 3),
                "throughput_ratio_points_vs_forward": round(t_f / t_p, 3),
                "density_tflops": round(P / 32 * FLOP_PER_32_POINTS / (t_d * 1e-3) / 1e12, 1),
                "density_fraction_of_2p5_pflops": round(P / 32 * FLOP_PER_32_POINTS / (t_d * 1e-3) / PEAK_FLOPS, 3),
                "forward_fraction_of_2p5_pflops": round(P / 32 * FLOP_PER_32_POINTS_FULL / (t_f * 1e-3) / PEAK_FLOPS, 3),
                "sigma_equals_forward_column_3": same,
            }
            print(json.dumps(row), flush=True)
            res["density"].append(row)
            del pts, out, sig_pts
            torch.cuda.empty_cache()
    # marching cubes at 512^3 on the fp16 sigma grid of the synthetic net.  Its sigma has no single object in it: a level
    # near the top of its range gives a surface of trained-scene size (a few million faces), the median level a stress case
    # with a face in most cells.
    r = 512
    R = (r, r, r)
    lo, step = mesh.grid_axes(R, bounds)
    sigma = mesh.density_grid(net, R, bounds, precision="fp16")
    sample = sigma.view(-1)[::97].float()
    t_dens = timed(lambda: mesh.density_grid(net, R, bounds, precision="fp16"), args.reps)
    res["marching_cubes"] = []
    for name, q in (("surface", 0.995), ("stress_median", 0.5)):
        level = float(torch.quantile(sample[:1 << 24], q))
        lvl = ctypes.c_float(level)
        ws = torch.empty(int(lib.nerf_amd_marching_cubes_workspace_bytes(*R)), dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        t_count = timed(lambda: lib.nerf_amd_marching_cubes_count(_lib.ptr(sigma), *R, lvl, _lib.ptr(ws), _lib.ptr(counts), st),
                        args.reps)
        nv, nf = (int(x) for x in counts.cpu())
        verts = torch.empty((nv, 3), device=dev)
        normals = torch.empty((nv, 3), device=dev)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        t_emit = timed(lambda: lib.nerf_amd_marching_cubes_emit(_lib.ptr(sigma), *R, lvl, f3(lo), f3(step), _lib.ptr(ws),
                                                                _lib.ptr(verts), _lib.ptr(normals), _lib.ptr(faces), nv, nf, st),
                       args.reps)
        del verts, normals, faces
        t_mc = timed(lambda: mesh.marching_cubes(sigma, level, bounds), args.reps)
        t_all = timed(lambda: mesh.extract_mesh(net, R, level, bounds, precision="fp16"), args.reps)
        n = r ** 3
        nblk = -(-n // 2048)
        # bytes each pass moves at least: sigma read once per pass; emit also writes the per-point first-vertex (4 B) and
        # edge-mask (1 B) words and reads them back in its face kernel, plus the mesh itself
        b_count = 4 * n + 8 * nblk
        b_emit = 2 * 4 * n + 2 * 5 * n + 24 * nv + 12 * nf + 16 * nblk
        row = {
            "case": name, "grid": r, "level_quantile": q, "level": level, "vertices": nv, "faces": nf,
            "count_ms": round(t_count, 3), "emit_ms": round(t_emit, 3), "marching_cubes_api_ms": round(t_mc, 3),
            "bytes_count_pass": b_count, "bytes_emit_pass": b_emit,
            "count_GBps": round(b_count / (t_count * 1e-3) / 1e9, 1), "emit_GBps": round(b_emit / (t_emit * 1e-3) / 1e9, 1),
            "density_grid_api_ms": round(t_dens, 3), "extract_mesh_ms": round(t_all, 3),
            "extraction_over_density": round(t_all / t_dens, 3),
        }
        print(json.dumps(row), flush=True)
        res["marching_cubes"].append(row)
        del ws
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
