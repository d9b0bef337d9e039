"""The argument rules of the C ABI (include/nerf_amd.h), pinned call by call: tests/golden/abi_refusals.json lists
(entry point, arguments, return value) triples recorded from the library.  Every call is refused (NERF_AMD_EINVAL = -1,
NERF_AMD_EUNSUP = -2), is an empty problem (0) or is a pure size query, so nothing is launched and no GPU is needed:
every pointer is NULL, a fake aligned address ("P") or a fake misaligned one (a number), and none is dereferenced.

The cases sit on both sides of each limit the entry points share (compositor backward N 512 / 513, masked and terminated
N 768 / 769, the sampler's Nc 2 / 3 / 256 / 257 and Nc + Nf 512 / 513, masked B 2^32 / 2^32 + 1, capacity 0 / 1 / B N /
B N + 1), and calls that break an EINVAL rule and an EUNSUP rule at once pin the ORDER in which an entry point applies
its rules.  On the passing side of a limit a later rule (a missing pointer) refuses the call, so the two sides differ
in their code wherever the ABI lets them; capacity = B N and B N + 1 are both -1, the rules behind that one being -1 too.

`python tests/test_abi_refusals_cpu.py` re-records the return values from the library in the tree."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals.json")
FAKE = 0x1000

with open(FIXTURE) as _f:
    CASES = json.load(_f)


def call(lib, case):
    return getattr(lib, case["fn"])(*[FAKE if a == "P" else a for a in case["args"]])


@pytest.fixture(scope="module")
def lib():
    from nerf_simple_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_fixture_covers_every_shared_limit():
    """Both sides of each limit are in the fixture for every entry point that applies it."""
    from nerf_simple_amd import _lib
    seen = {}
    for c in CASES:
        assert c["fn"] in _lib._SIGNATURES and len(c["args"]) == len(_lib._SIGNATURES[c["fn"]][1]), c
        seen.setdefault(c["fn"][len("nerf_amd_"):], set()).update(a for a in c["args"] if isinstance(a, int))
    for fn in ("volume_render_backward", "volume_render_rays_backward", "volume_render_mse_backward",
               "volume_render_masked_backward", "occupancy_points_capped", "volume_render_masked_mse_backward"):
        assert {512, 513} <= seen[fn], fn
    for fn in ("occupancy_mask_words", "occupancy_mark", "occupancy_points", "volume_render_masked",
               "volume_render_masked_pixels", "volume_render_masked_backward", "termination_advance"):
        assert {768, 769, 2 ** 32, 2 ** 32 + 1} <= seen[fn], fn
    for fn in ("sample_pdf", "volume_render_mse_backward_pdf", "render_hierarchical_forward",
               "volume_render_masked_mse_backward_pdf"):
        assert {2, 3, 256, 257} <= seen[fn], fn
    for fn in ("occupancy_points_capped", "volume_render_masked_mse_backward", "volume_render_masked_mse_backward_pdf"):
        assert {0, 1, 4 * 64, 4 * 64 + 1, 2 ** 32, 2 ** 32 + 1} <= seen[fn], fn
    two_rules = {}
    for c in CASES:
        if c["note"].startswith("two rules:"):
            two_rules[c["fn"]] = two_rules.get(c["fn"], 0) + 1
    refusing = {c["fn"] for c in CASES if not c["fn"].endswith(("_workspace_bytes", "_forward", "_forward_rays"))}
    refusing.add("nerf_amd_render_hierarchical_forward")
    for fn in refusing:
        assert two_rules.get(fn, 0) >= 2, fn


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: f"{CASES[i]['fn'][len('nerf_amd_'):]}-{i}")
def test_abi_refusal(lib, i):
    case = CASES[i]
    assert call(lib, case) == case["expect"], (case["fn"], case["note"], case["args"])


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    from nerf_simple_amd import _lib
    for c in CASES:
        c["expect"] = call(_lib.lib(), c)
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in CASES) + "\n]\n")
    print(f"{len(CASES)} cases recorded")
