#!/usr/bin/env python3
"""Do the masked backward and its heads write the bytes another build of the library writes?

    python tools/masked_head_bytes.py --parent /path/to/other/libnerf_amd.so > profiles/<name>_bytes.txt

Both libraries are loaded with ctypes in one process and the four entry points that run the masked compositor's backward walk
(csrc/occupancy_train.hip) are called on the same inputs, so that thirteen of the kernel's twenty-five instantiations run (the
other twelve, the pair's coarse head with a control on, are compared with their chain of stages bit for bit by
tests/test_gpu_pair_controls.py):
  nerf_amd_volume_render_masked_backward           the five gradients, all given
  nerf_amd_volume_render_masked_mse_backward       the MSE head under the clamp
  nerf_amd_volume_render_masked_mse_backward_pdf   ... with the sampler, Nf = 3, 64, 128, 256 and 512 - N (keys per lane 1, 1, 2,
                                                   4, 8; N + Nf <= 512 is the sampler's limit)
  nerf_amd_volume_render_masked_mse_backward_dist  ... with every combination of noise, background and distortion, the noise
                                                   seed in the argument and in memory, loss_ray given and NULL
B = 5 and 37; N = 1, 3, 65, 130 (the sampler from 3 on); the sparse mask of tests/test_gpu_ray_routines.py (ray 0 dead, ray 1
live at its last sample only, the others where (7 i + 3 ray) % 5 < 2); C = P' + 3, P', P' - 3 and 1 where 1 <= C <= B N.
Every output buffer (d_raw_live[C, 4], rgb, loss_ray, ts_out, 32 guard bytes behind each) is filled with 0xFF in front of the
call and compared byte for byte.  Exit status 1 when a byte or a return code differs."""
import argparse
import ctypes
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_simple_amd import _lib                                                        # noqa: E402

FNS = ("nerf_amd_volume_render_masked_backward", "nerf_amd_volume_render_masked_mse_backward",
       "nerf_amd_volume_render_masked_mse_backward_pdf", "nerf_amd_volume_render_masked_mse_backward_dist")
GUARD = 32


def load(path):
    h = ctypes.CDLL(path)
    for name in FNS:
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return h


def sparse_mask(B, N):
    s = np.arange(N)
    live = np.zeros((B, N), bool)
    live[1, N - 1] = True
    for r in range(2, B):
        live[r] = (7 * s + 3 * r) % 5 < 2
    words = np.zeros((B, (N + 63) // 64), np.uint64)
    for r, k in zip(*np.nonzero(live)):
        words[r, k // 64] |= np.uint64(1) << np.uint64(k % 64)
    return live, words.view(np.int64), np.concatenate([[0], np.cumsum(live.sum(1))]).astype(np.int64)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", required=True, help="the other build's libnerf_amd.so")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the kernels run on the GPU"
    dev = torch.device("cuda:0")
    libs = (load(args.parent), load(_lib.LIB_PATH))
    st, ptr = _lib.stream_ptr(dev), _lib.ptr
    calls = buffers = nbytes = differ = 0

    def run(what, fn, build, outs):
        """Call `fn` of both libraries with build(out pointers...) and compare the `outs` (name -> floats) byte for byte."""
        nonlocal calls, buffers, nbytes, differ
        got = []
        for h in libs:
            bufs = {k: torch.full((4 * n + GUARD,), 0xFF, dtype=torch.uint8, device=dev) for k, n in outs.items() if n is not None}
            rc = getattr(h, fn)(*build({k: ptr(bufs[k]) if k in bufs else None for k in outs}))
            torch.cuda.synchronize(dev)
            got.append((rc, bufs))
        calls += 1
        (rc_a, a), (rc_b, b) = got
        if rc_a != 0 or rc_b != 0:
            print(f"DIFFER {what}: return codes {rc_a} (parent) {rc_b} (this tree)")
            differ += 1
            return
        for k in a:
            buffers += 1
            nbytes += a[k].numel()
            assert bool((a[k][-GUARD:] == 0xFF).all()), (what, k, "the parent wrote behind its buffer")
            if not torch.equal(a[k], b[k]):
                differ += 1
                print(f"DIFFER {what}: {k}, {int((a[k] != b[k]).sum())} bytes")

    for B, N in itertools.product((5, 37), (1, 3, 65, 130)):
        gen = torch.Generator().manual_seed(9000 + 131 * B + N)
        live, words, offs = sparse_mask(B, N)
        P = int(offs[-1])
        raw = torch.randn(P, 4, generator=gen)
        raw[:, 3] = 15.0 * raw[:, 3] + 7.5
        ts = torch.sort(2.0 + 4.0 * torch.rand(B, N, generator=gen), dim=1).values
        rays, gt, bg = torch.randn(B, 6, generator=gen), torch.rand(B, 3, generator=gen), torch.rand(B, 3, generator=gen)
        grads = [torch.randn(*shape, generator=gen) for shape in ((B, 3), (B,), (B, N), (B,), (B, N))]
        u_f = torch.rand(B, 512, generator=gen)
        raw, ts, rays, gt, bg, u_f, *grads = [x.contiguous().to(dev) for x in (raw, ts, rays, gt, bg, u_f, *grads)]
        mask, offsets = torch.from_numpy(words).to(dev), torch.from_numpy(offs).to(dev)
        step = torch.tensor([3], dtype=torch.int64, device=dev)          # the noise seed's offset in memory
        jit = (ptr(rays), ptr(ts), None, _lib.FLAG_TS_GIVEN, 0, 11, ptr(mask), ptr(offsets))
        run(f"five gradients B={B} N={N}", FNS[0],
            lambda o: (ptr(raw), *jit, *[ptr(g) for g in grads], o["d_raw_live"], B, N, st), {"d_raw_live": 4 * P})
        for C in sorted({c for c in (P + 3, P, P - 3, 1) if 1 <= c <= B * N}):
            where = f"B={B} N={N} P'={P} C={C}"
            run(f"mse head {where}", FNS[1],
                lambda o: (ptr(raw), *jit, ptr(gt), o["rgb"], o["d_raw_live"], C, B, N, st), {"rgb": 3 * B, "d_raw_live": 4 * C})
            for Nf in (3, 64, 128, 256, 512 - N) if N >= 3 else ():
                u = u_f[:, :Nf].contiguous()
                run(f"pdf head E={1 if Nf <= 64 else 2 if Nf <= 128 else 4 if Nf <= 256 else 8} Nf={Nf} {where}", FNS[2],
                    lambda o: (ptr(raw), *jit, ptr(gt), ptr(u), o["rgb"], o["d_raw_live"], o["ts_out"], C, B, N, Nf, st),
                    {"rgb": 3 * B, "d_raw_live": 4 * C, "ts_out": B * (N + Nf)})
            for noise, with_bg, dist, in_mem, with_loss in itertools.product((0, 1), repeat=5):
                if in_mem and not noise:
                    continue
                stride = 3 if B == 37 else 0
                run(f"controls noise={noise} bg={with_bg} dist={dist} seed_mem={in_mem} loss_ray={with_loss} {where}", FNS[3],
                    lambda o: (ptr(raw), *jit, ptr(gt), ptr(bg) if with_bg else None, stride, 0.75 if noise else 0.0,
                               _lib.FLAG_SEED_IN_MEMORY if in_mem else 0, 77, ptr(step) if in_mem else None, 6.5,
                               0.01 / (4.0 * B) if dist else 0.0, o["rgb"], o["loss_ray"], o["d_raw_live"], C, B, N, st),
                    {"rgb": 3 * B, "loss_ray": B if with_loss else None, "d_raw_live": 4 * C})
    print(f"{calls} calls of each library, {buffers} buffers, {nbytes} bytes compared, {differ} differ")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
