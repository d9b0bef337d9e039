"""The training controls' rule, stated once: the flat keywords and the ``Controls`` bundle resolve to the
same record, each refusal's sentence is written in one place, and utils/controls.py is a leaf.  No GPU: the records are
resolved on the CPU device and the rest reads the sources."""
import ast
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-simple_amd")
B, CPU = 2, torch.device("cpu")


def _same(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return True
    for name, x, y in zip(a._fields, a, b):
        if torch.is_tensor(x) or torch.is_tensor(y):
            assert torch.is_tensor(x) and torch.is_tensor(y) and x.dtype == y.dtype == torch.float32, name
            assert x.shape == y.shape and torch.equal(x, y), name
        else:
            assert type(x) is type(y) and x == y, (name, x, y)
    return True


PER_RAY = torch.tensor([[0.1, 0.2, 0.3], [0.9, 0.8, 0.7]])
CASES = {
    "scalar background": dict(background=(0.2, 0.4, 0.6)),
    "per-ray background": dict(background=PER_RAY),
    "noise only": dict(sigma_noise=0.5, noise_seed=11),
    "distortion only": dict(distortion=0.01),
    "all three": dict(background=PER_RAY, sigma_noise=0.5, noise_seed=11, distortion=0.01),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_flat_keywords_and_bundle_resolve_to_the_same_record(case):
    from nerf_simple_amd.training import Controls
    from nerf_simple_amd.utils import controls as C
    kw = CASES[case]
    bundle = C.resolve(C.from_keywords(Controls(**kw), {"occupancy": None}), B, CPU, 5)
    flat = C.resolve(C.from_keywords(None, {"occupancy": None}, **kw), B, CPU, 5)
    assert isinstance(bundle, C.Resolved) and _same(bundle, flat)
    assert bundle._fields == ("bg", "stride", "std", "noise_seed", "noise_ray_id0", "lam")
    want_bg = kw.get("background")
    assert (bundle.bg is None) == (want_bg is None) and bundle.stride == (0 if want_bg is None or len(want_bg) == 3 else 3)
    if want_bg is not None:
        assert torch.equal(bundle.bg, torch.as_tensor(want_bg, dtype=torch.float32))
    assert (bundle.std, bundle.noise_seed, bundle.noise_ray_id0, bundle.lam) == (
        kw.get("sigma_noise", 0.0), kw.get("noise_seed", 0), 5, kw.get("distortion", 0.0))
    with pytest.raises(AttributeError):
        bundle.std = 1.0                                             # immutable


def test_the_fine_record_differs_in_the_noise_seed_alone():
    from nerf_simple_amd import training as T
    from nerf_simple_amd.utils import controls as C
    for seed in (0, 11, (1 << 63) + 5, (1 << 64) - 1):
        c = C.pair(T.Controls(background=PER_RAY, sigma_noise=0.5, noise_seed=seed), "a test")
        coarse = C.resolve(c, B, CPU, 3)
        fine = coarse.fine()
        assert fine.noise_seed == (seed + T.FINE_NOISE_OFFSET) % (1 << 64) and fine.noise_seed != coarse.noise_seed
        assert fine._replace(noise_seed=coarse.noise_seed) == coarse and fine.bg is coarse.bg


def test_everything_off_resolves_to_none():
    from nerf_simple_amd.training import Controls
    from nerf_simple_amd.utils import controls as C
    assert C.resolve(None, B, CPU) is None
    assert C.resolve(Controls(), B, CPU) is None and C.resolve(Controls(noise_seed=7), B, CPU) is None
    assert C.from_keywords(None, {"occupancy": object()}) is None
    assert C.from_keywords(None, {"occupancy": None}, noise_seed=7) is None
    assert C.pair(None, "a test") is None and C.pair(Controls(noise_seed=7), "a test") is None


# one distinctive literal of each rule's sentence (section 37 lists them)
RULES = (
    "controls must be a training.Controls",
    "and the flat keywords background / sigma_noise / noise_seed / distortion say the same thing",
    "background must be one colour [3] or one per ray",
    "is a training regulariser, not a render option",
    "the distortion term belongs to a training step",
    "serve the dense path only: not with",
    "distortion serves the dense and guided steps only",
    "is not offered on the coarse + fine pair",
    "controls= serves the dense and the masked single-network steps",
    "controls= does not reach the terminated render yet",
)


def _sources():
    out = {}
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py"):
                path = os.path.join(d, f)
                out[os.path.relpath(path, PKG)] = open(path).read()
    return out


def test_each_rule_is_written_once():
    """Each rule's sentence occurs as a literal exactly once in the package's Python, in utils/controls.py (the type check and the
    'same thing' ValueError are the two halves of the first rule)."""
    sources = _sources()
    for rule in RULES:
        counts = {f: t.count(rule) for f, t in sources.items() if rule in t}
        assert counts == {os.path.join("utils", "controls.py"): 1}, (rule, counts)


def test_controls_is_a_leaf():
    """utils/controls.py imports ``_lib`` and torch (and the standard library): neither rendering nor training, at the top or
    inside a function."""
    tree = ast.parse(open(os.path.join(PKG, "utils", "controls.py")).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names |= {f"{'.' * node.level}{node.module or ''}:{a.name}" for a in node.names}
    assert names == {"math", "torch", "typing:NamedTuple", "typing:Optional", "..:_lib"}, names
