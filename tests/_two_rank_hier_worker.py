"""Worker of tests/test_gpu_multirank_hierarchical.py: one rank of a 2-rank job on ONE GPU (gloo rendezvous, both ranks
on cuda:0) training the hierarchical coarse + fine pair data-parallel, eagerly and as captured graphs.  Each rank takes
its half of golden G6's rays and of the fixed jitter; results go to the directory in argv[1]."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NC, NF = 64, 128


def pair_inputs():
    """(rays, gt, u_c, u_f) of the global batch: G6's rays, targets and coarse jitter, fine jitter from a fixed seed."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "train.npz"))
    rays, gt, u_c = (torch.from_numpy(np.ascontiguousarray(g[k])) for k in ("rays", "gt", "u"))
    u_f = torch.rand(rays.shape[0], NF, generator=torch.Generator().manual_seed(21))
    return rays, gt, u_c, u_f


def main():
    out_dir = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    from nerf_simple_amd import _lib, parallel
    from nerf_simple_amd.optim import FusedAdam
    from nerf_simple_amd.training import GraphedHierarchicalTrainStep, train_step_hierarchical
    from nerf_simple_amd.utils import synthetic
    from nerf_simple_amd.utils.nets import Nerf
    _lib.lib()
    rays, gt, u_c, u_f = pair_inputs()
    half = rays.shape[0] // world
    sl = slice(rank * half, (rank + 1) * half)
    args = [x[sl].to(dev) for x in (rays, gt, u_c, u_f)]

    def fresh():
        nets = []
        for s in (0, 1):
            n = Nerf(precision="bf16").to(dev)
            n.load_state_dict(synthetic.synthetic_state_dict(s, "default"))
            parallel.broadcast_parameters(n)
            nets.append(n)
        return nets, FusedAdam(nets, lr=5e-4)

    res = {}
    # eager: one all-reduce of the two networks' gradients as one bucket
    (net_c, net_f), opt = fresh()
    loss = train_step_hierarchical(net_c, net_f, opt, args[0], args[1], NC, NF, u_c=args[2], u_f=args[3],
                                   group=dist.group.WORLD)
    res["eager_grads"] = torch.cat([p.grad.reshape(-1) for p in opt.params]).cpu().numpy()
    res["eager_loss"] = np.array([float(loss)])
    res["eager_params"] = opt.flat.cpu().numpy()
    # graphed: the combined 1,191,688-element vector all-reduced between graph A and graph B
    (net_c, net_f), opt = fresh()
    stepper = GraphedHierarchicalTrainStep(net_c, net_f, opt, half, NC, NF, group=dist.group.WORLD)
    assert stepper.exchange and stepper.graph_ab is None
    loss = stepper.step(args[0], args[1], u_c=args[2], u_f=args[3])
    torch.cuda.synchronize()
    res["graphed_grads"] = stepper.grads.cpu().numpy()
    res["graphed_loss"] = np.array([float(loss)])
    res["graphed_params"] = opt.flat.cpu().numpy()
    for _ in range(2):
        stepper.step(args[0], args[1], u_c=args[2], u_f=args[3])
    torch.cuda.synchronize()
    res["graphed_params3"] = opt.flat.cpu().numpy()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
