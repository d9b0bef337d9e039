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


def masked_backward_instantiations(kernels):
    """[(upstream, E)] of the masked_backward_kernel<Up, E> symbols among `kernels`, sorted."""
    found = []
    for name in kernels:
        m = re.search(r"masked_backward_kernelIN14nerf_composite\d+(FiveGrads|LossHeadILb0ELb0ELb0EE)ELi(\d+)EEEv", name)
        if m:
            found.append(("FiveGrads" if m.group(1) == "FiveGrads" else "MseHead", int(m.group(2))))
    return sorted(found)
