"""The jitter source rule and the entry points' argument rules, each stated once, without a GPU.

``host_rng.reference_rand`` is replaced by a recorder that hands out CPU tensors and logs every draw and every ``finish()``;
``_lib.require_cuda_f32`` is relaxed to accept CPU float32.  ``jitter.single`` and ``jitter.pair`` are then walked through their
whole argument lattice: the flags, WHICH tensor comes back (identity) and the exact sequence of draws are asserted.
"""
import itertools
import os
import re
from types import SimpleNamespace

import pytest
import torch

from nerf_simple_amd import _lib, training
from nerf_simple_amd.utils import host_rng, jitter, rendering

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, NC = 7, 5, 5
TS, RNG = _lib.FLAG_TS_GIVEN, _lib.FLAG_DEVICE_RNG


class _Pending:
    def __init__(self, log, shape):
        self.log, self.shape = log, shape

    def finish(self):
        self.log.append(("finish", self.shape))


@pytest.fixture
def draws(monkeypatch):
    """The recorder: [('draw', (B, N)) | ('finish', (B, N)), ...] in call order, and the tensors handed out."""
    log, made = [], []

    def reference_rand(b, n, device):
        log.append(("draw", (b, n)))
        made.append(torch.full((b, n), float(len(made))))
        return made[-1], _Pending(log, (b, n))

    def require_f32(t, name):
        if not torch.is_tensor(t):
            raise AssertionError(f"{name} needs to be a torch tensor")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32, got {t.dtype}")
        return t

    monkeypatch.setattr(host_rng, "reference_rand", reference_rand)
    monkeypatch.setattr(_lib, "require_cuda_f32", require_f32)
    return SimpleNamespace(log=log, made=made)


@pytest.mark.parametrize("has_u, has_ts, device_rng", itertools.product((False, True), repeat=3))
def test_single_lattice(draws, has_u, has_ts, device_rng):
    """Precedence ts > u > device_rng > one CPU draw, which comes back unfinished."""
    u = torch.rand(B, N) if has_u else None
    ts = torch.rand(B, N) if has_ts else None
    jit, flags, pending = jitter.single(B, N, "cpu", u=u, ts=ts, device_rng=device_rng)
    if has_ts:
        assert jit is ts and flags == TS and pending is None and draws.log == []
    elif has_u:
        assert jit is u and flags == 0 and pending is None and draws.log == []
    elif device_rng:
        assert jit is None and flags == RNG and pending is None and draws.log == []
    else:
        assert jit is draws.made[0] and flags == 0 and draws.log == [("draw", (B, N))]        # not finished: the caller's
        pending.finish()
        assert draws.log == [("draw", (B, N)), ("finish", (B, N))]


@pytest.mark.parametrize("has_uc, has_uf, device_rng, Nf", itertools.product((False, True), (False, True), (False, True), (0, 3)))
def test_pair_lattice(draws, has_uc, has_uf, device_rng, Nf):
    """A given u_c wins over device_rng; u_c then u_f, each finished at once; u_f drawn only when absent without device_rng
    -- at Nf == 0 too (the draw of [B, 0] is reference_rand's business: it takes nothing from the generator)."""
    u_c = torch.rand(B, NC) if has_uc else None
    u_f = torch.rand(B, Nf) if has_uf else None
    jit_c, flags, out_f = jitter.pair(B, NC, Nf, "cpu", u_c=u_c, u_f=u_f, device_rng=device_rng)
    want, made = [], iter(draws.made)
    if has_uc:
        assert jit_c is u_c and flags == 0
    elif device_rng:
        assert jit_c is None and flags == RNG
    else:
        want += [("draw", (B, NC)), ("finish", (B, NC))]
        assert jit_c is next(made) and flags == 0
    if has_uf:
        assert out_f is u_f
    elif device_rng:
        assert out_f is None
    else:
        want += [("draw", (B, Nf)), ("finish", (B, Nf))]
        assert out_f is next(made)
    assert draws.log == want


def test_given_jitter_is_made_contiguous(draws):
    u = torch.rand(N, B).t()
    jit, flags, _ = jitter.single(B, N, "cpu", u=u)
    assert jit.is_contiguous() and torch.equal(jit, u) and flags == 0


@pytest.mark.parametrize("bad", ("shape", "dtype", "type"))
def test_refused_before_any_draw(draws, bad):
    wrong = {"shape": torch.rand(B, N + 1), "dtype": torch.rand(B, N).double(), "type": [[0.0] * N] * B}[bad]
    err = {"shape": RuntimeError, "dtype": RuntimeError, "type": AssertionError}[bad]
    msg = {"shape": r"^u / ts must be \[B, N\]$", "dtype": r"^{} must be float32, got torch.float64$",
           "type": r"^{} needs to be a torch tensor$"}[bad]
    for kw in ("u", "ts"):
        with pytest.raises(err, match=msg.format(kw)):
            jitter.single(B, N, "cpu", **{kw: wrong})
        with pytest.raises(err, match=msg.format(kw)):
            jitter.check(B, N, **{kw: wrong})
    # the pair: u_c absent (it would be drawn first), u_f wrong -- nothing is drawn
    msg = {"shape": rf"^{{}} must be \[B, {N}\]$", "dtype": r"^{} must be float32, got torch.float64$",
           "type": r"^{} needs to be a torch tensor$"}[bad]
    with pytest.raises(err, match=msg.format("u_f")):
        jitter.pair(B, NC, N, "cpu", u_f=wrong)
    with pytest.raises(err, match=msg.format("u_c")):
        jitter.pair(B, N, 3, "cpu", u_c=wrong)
    assert draws.log == []


def test_shape_left_to_the_entry_point(draws):
    """render_view, sample_pdf and ProposalVolume.sample pass shape_error=None: the dtype is still looked at, the shape is theirs."""
    u = torch.rand(B, N + 1)
    assert jitter.single(B, N, "cpu", u=u, shape_error=None)[0] is u
    with pytest.raises(RuntimeError, match="^u_c must be float32"):
        jitter.single(B, N, "cpu", u=u.double(), names=("u_c", "ts_c"), shape_error=None)
    assert draws.log == []


def test_tbins_follow_the_flags():
    assert jitter.tbins(2, 6, N, "cpu", TS) is None and jitter.tbins(2, 6, N, "cpu", TS | RNG) is None
    assert torch.equal(jitter.tbins(2, 6, N, "cpu", RNG), torch.linspace(2, 6, N + 1))
    assert jitter.tbins(2, 6, N, "cpu", 0) is rendering._tbins(2, 6, N, "cpu")


# ---- the argument rules: every message against the literal string the entry points raised before they shared one -------------
def test_require_messages(draws):
    assert _lib.require_rays(torch.zeros(B, 6)) == B
    for rays in (torch.zeros(B, 5), torch.zeros(6), torch.zeros(B, 6, 1)):
        with pytest.raises(RuntimeError, match=r"^rays must be \[B, 6\]$"):
            _lib.require_rays(rays)
    with pytest.raises(RuntimeError, match=r"^rays must be float32, got torch.float64$"):
        _lib.require_rays(torch.zeros(B, 6).double())

    t = torch.zeros(B, NC)
    assert _lib.require_shape(t, "u_c", (B, NC)) is t and _lib.require_shape(None, "u_c", (B, NC)) is None
    with pytest.raises(RuntimeError, match=r"^ts_c must be \[B, 4\]$"):
        _lib.require_shape(t, "ts_c", (B, 4))
    with pytest.raises(RuntimeError, match=r"^u_f must be \[B, 5\]$"):
        _lib.require_shape(torch.zeros(B + 1, NC), "u_f", (B, NC))

    cpu, gpu = torch.device("cpu"), torch.device("cuda", 0)
    _lib.require_same_device("occupancy grid", SimpleNamespace(device=gpu), gpu)
    with pytest.raises(RuntimeError, match=r"^the occupancy grid lives on cpu, the rays on cuda:0$"):
        _lib.require_same_device("occupancy grid", SimpleNamespace(device=cpu), gpu)
    with pytest.raises(RuntimeError, match=r"^the proposal volume lives on cuda:0, the rays on cpu$"):
        _lib.require_same_device("proposal volume", SimpleNamespace(device=gpu), cpu)

    for Nc, Nf in ((3, 0), (256, 256), (5, 3)):
        _lib.require_pair_sizes(Nc, Nf)
    for Nc, Nf in ((2, 3), (257, 0), (5, -1), (256, 257)):
        with pytest.raises(ValueError, match=re.escape(f"hierarchical sampling needs 3 <= Nc <= 256 and Nc + Nf <= 512 (got Nc={Nc}, "
                                                       f"Nf={Nf})")):
            _lib.require_pair_sizes(Nc, Nf)

    net = SimpleNamespace(precision="fp16")
    assert _lib.precision_of(net, None) == _lib.FP16 and _lib.precision_of(net, "bf16") == _lib.BF16
    with pytest.raises(ValueError, match=r"^precision must be 'fp32', 'bf16' or 'fp16', got 'int8'$"):
        _lib.precision_of(net, "int8")

    assert training._check_guided is rendering._check_guided
    with pytest.raises(TypeError, match=r"^proposal must be a ProposalVolume \(utils/proposal.py\)$"):
        rendering._check_guided(net, object())


def test_workspace():
    assert _lib.workspace(0, "cpu").numel() == 256 and _lib.workspace(300, "cpu").numel() == 300
    assert _lib.workspace(0, "cpu", floor=0) is None and _lib.workspace(300, "cpu", floor=0).numel() == 300
    assert _lib.workspace(300, "cpu").dtype == torch.uint8


def test_one_copy_of_each_rule():
    """The greps of section 31: each rule's text appears once in the package, and only jitter.py draws from host_rng."""
    pkg = os.path.join(ROOT, "nerf-simple_amd")
    src = {}
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                with open(os.path.join(d, f)) as fh:
                    src[os.path.relpath(os.path.join(d, f), pkg)] = fh.read()

    def hits(text):
        return sorted(k for k, v in src.items() for _ in range(v.count(text)))

    assert hits("rays must be [B, 6]") == ["_lib.py"]
    assert hits("lives on {tensor.device}, the rays on") == ["_lib.py"] and hits(", the rays on") == ["_lib.py"]
    assert hits("precision_code(net.precision if") == ["_lib.py"]
    assert hits("precision_code(self.precision if") == hits("precision_code(net_c.precision if") == []
    assert hits("hierarchical sampling needs 3 <= Nc <= 256") == ["_lib.py"]
    assert hits("u / ts must be [B, N]") == [os.path.join("utils", "jitter.py")]
    assert hits("proposal must be a ProposalVolume") == [os.path.join("utils", "rendering.py")]
    assert sorted(set(hits("reference_rand("))) == [os.path.join("utils", "host_rng.py"), os.path.join("utils", "jitter.py")]
    assert hits("def _jitter") == [] and hits("def _tb(") == []
