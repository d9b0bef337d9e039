"""The hierarchical coarse + fine training step under a process group: two ranks share the one test GPU (gloo rendezvous
on 127.0.0.1), each takes half the batch, and the averaged combined gradient of both networks must be the single-process
gradient of the full batch -- eager (train_step_hierarchical) and graphed (GraphedHierarchicalTrainStep)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def two_rank_pair(tmp_path_factory):
    assert torch.cuda.is_available()
    out = tmp_path_factory.mktemp("two_rank_hier")
    port = free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_two_rank_hier_worker.py"), str(out)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=600)[0].decode(errors="replace") for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    return np.load(out / "rank0.npz"), np.load(out / "rank1.npz")


def test_pair_data_parallel_step_equals_global_batch(two_rank_pair):
    """Both ranks' averaged gradient (coarse then fine, one vector) equals the full-batch gradient of one process up to
    the float atomics' summation order (the bound of test_data_parallel_step_equals_global_batch); the mean of the rank
    losses is the global loss; both ranks end with identical parameters, in the eager and the graphed form."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _two_rank_hier_worker import NC, NF, pair_inputs
    from nerf_simple_amd.training import train_step_hierarchical
    from nerf_simple_amd.utils import synthetic
    from nerf_simple_amd.utils.nets import Nerf
    r0, r1 = two_rank_pair
    dev = torch.device("cuda:0")
    rays, gt, u_c, u_f = (x.to(dev) for x in pair_inputs())
    nets = []
    for s in (0, 1):
        n = Nerf(precision="bf16").to(dev)
        n.load_state_dict(synthetic.synthetic_state_dict(s, "default"))
        nets.append(n)
    opt = torch.optim.SGD(list(nets[0].parameters()) + list(nets[1].parameters()), lr=0.0)
    loss = float(train_step_hierarchical(nets[0], nets[1], opt, rays, gt, NC, NF, u_c=u_c, u_f=u_f))
    want = torch.cat([p.grad.reshape(-1) for n in nets for p in n.parameters()]).cpu().numpy()
    assert want.size == 1191688
    for form in ("eager", "graphed"):
        got = r0[f"{form}_grads"]
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{form}: max |averaged - full batch| / max |g| = {err:.3e}")
        assert err <= 2e-5, (form, err)
        assert abs(0.5 * (float(r0[f"{form}_loss"][0]) + float(r1[f"{form}_loss"][0])) - loss) <= 1e-5 * loss, form
        assert np.array_equal(r0[f"{form}_params"], r1[f"{form}_params"]), form
    assert np.array_equal(r0["graphed_params3"], r1["graphed_params3"]) and np.isfinite(r0["graphed_params3"]).all()
    assert not np.array_equal(r0["graphed_params3"], r0["graphed_params"])
