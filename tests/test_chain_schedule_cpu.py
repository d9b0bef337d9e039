"""tools/stamp_tiles.py --chunk-barriers / --prio-younger: the insertion points of the chunk-barrier stamps and of the
diagnostic static priority are matched literally in csrc/mlp_bf16_16.hip and csrc/mlp16_chain.h; this keeps them in step
with the sources, and checks that neither the stamps nor a wave-id test reach the shipped files."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool():
    spec = importlib.util.spec_from_file_location("stamp_tiles", os.path.join(ROOT, "tools", "stamp_tiles.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_chunk_barrier_stamps_find_their_insertion_points():
    mod = load_tool()
    src = mod.stamped_source(chunk_barriers=True, prio_younger=True)      # SystemExit when a pattern is missing or ambiguous
    assert src.count("g_cwait") == 4 and src.count("nerf_amd_debug_read_chunk_waits") == 1
    assert src.count("__builtin_amdgcn_s_setprio(1)") == 1 and "readfirstlane(threadIdx.x) >= 256" in src
    chain = mod.stamped_chain(chunk_barriers=True)
    assert chain.count("__builtin_amdgcn_s_memtime()") == 2               # one in front of the chunk barrier, one behind
    # the fp16 plan the tool labels its table with: 34 chunks, 2088 MFMAs per wave and tile
    assert sum(n for _, n, _ in mod.FP16_CHUNKS) == 34 and sum(n * m for _, n, m in mod.FP16_CHUNKS) == 2088
    assert mod.CW_N >= 38


def test_shipped_chain_carries_no_stamp_and_no_wave_test():
    mod = load_tool()
    shipped = mod.stamped_chain(False)
    assert shipped == open(os.path.join(ROOT, "nerf-simple_amd", "csrc", "mlp16_chain.h")).read()
    assert "s_memtime" not in shipped and "cw_t0" not in shipped
    # the priority schedule is the same code in every wave
    body = shipped[shipped.index("constexpr int BARRIER_TAIL"):shipped.index("struct Ctx")]
    assert "threadIdx" not in body and "wave" not in body.replace("waves", "")
