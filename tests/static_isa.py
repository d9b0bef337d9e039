"""The static ISA checks of the masked sources, shared by the CPU tests that name their kernels
(test_occupancy_training_cpu.py, test_occupancy_graphed_cpu.py, test_occupancy_hierarchical_cpu.py): tools/check_vmcnt.py
on one source of csrc/ -- no counted vmcnt wait is short, no wide store has its data registers overwritten by the next
instruction (the store-data hazard of csrc/nerf_device.h store_granule), and no kernel uses an atomic (every output row is
written by exactly one lane).  A source is assembled once per process."""
import functools
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def checked_kernels(source):
    """{kernel symbol: lines} of csrc/<source>, every kernel checked."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_vmcnt
    finally:
        sys.path.pop(0)
    asm = check_vmcnt.assemble(os.path.join(ROOT, "nerf-simple_amd", "csrc", source))
    kernels = check_vmcnt.kernels_of(asm)
    for name, lines in kernels.items():
        checked, bad = check_vmcnt.check_kernel(lines)
        assert not bad, (name, bad[:5])
        n, offenders = check_vmcnt.check_store_data_hazard(lines)
        assert not offenders, (name, offenders[:3])
        text = "\n".join(lines) if not isinstance(lines, str) else lines
        assert "atomic" not in text, name
    return kernels


_MASKED = re.compile(r"masked_backward_kernelIN14nerf_composite\d+(FiveGrads|LossHeadILb([01])ELb([01])ELb0EE)ELb([01])ELi(\d+)EEEv")


def masked_backward_instantiations(kernels):
    """[(upstream, E)] of the masked_backward_kernel<Up, false, E> symbols with a plain upstream among `kernels`, sorted."""
    found = []
    for m in filter(None, map(_MASKED.search, kernels)):
        if m.group(4) == "0" and m.group(2) in (None, "0") and m.group(3) in (None, "0"):
            found.append(("FiveGrads" if m.group(1) == "FiveGrads" else "MseHead", int(m.group(5))))
    return sorted(found)


def masked_term_instantiations(kernels):
    """[(NOISE, BG, DIST, E)] of the masked_backward_kernel<LossHead<BG, DIST, false>, NOISE, E> symbols with a term on, sorted."""
    found = []
    for m in filter(None, map(_MASKED.search, kernels)):
        if m.group(1) != "FiveGrads" and "1" in (m.group(2), m.group(3), m.group(4)):
            found.append((int(m.group(4)), int(m.group(2)), int(m.group(3)), int(m.group(5))))
    return sorted(found)
