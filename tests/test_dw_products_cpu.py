"""CPU tests of csrc/dw_products.h -- the table of the 14 dW products, the bucket rule, the split of the workgroups over the
products and the layout of the e4m3 scratch, shared by csrc/dw_gemm.hip and csrc/dw_gemm_f8.hip -- against the tests' own
statements of the same things: tests/train_chain_model.py (which operand pairs give which tensor, OFFSETS) and
tests/storage_model.py (PRODUCT_WIDTHS, workgroup_shares, narrow_offsets), both written before the header and not derived
from it.  tests/dw_products_dump.cpp prints the header as JSON; it is compiled with g++ and run as a child process: no GPU, no
HIP, nothing loaded into Python."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import storage_model as S
import test_gpu_train_chain as T
import train_chain_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"bf16": S.BF16_FORM, "e4m3": S.E4M3_FORM}
CUS = (1, 8, 256, 304)
# where ``need`` first exceeds 1 (2^21 points at 2 bytes per feature, 2^22 at 1) and where it exceeds the smallest ideal share
LARGE = (2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1, 2 ** 22 - 1, 2 ** 22, 2 ** 22 + 1, 2 ** 24 + 5, 2 ** 26 + 1)
SIZES = tuple(sorted(set(S.INT_SIZES) | set(T.INT_SIZES) | set(LARGE)))
SCRATCH_SIZES = (0, 1, 1000, 4097)

DY, ACT = (lambda L: ("DY", L)), (lambda L: ("ACT", L))
POSX, POSD, DSR = ("POSX", 0), ("POSD", 0), ("DSR", 0)
# the operand pairs of train_chain_model.expected_param_grads, by state-dict name:
# (A, B, first row of A^T B stored, rows stored, first column of the tensor, columns stored)
PAIRING = {
    "layers_0.0.weight": [(DY(0), POSX, 0, 256, 0, 63)],                                           # dY[0]^T posx[:, :63]
    **{M.LAYER_NAMES[L] + ".weight": [(DY(L), ACT(L - 1), 0, 256, 0, 256)] for L in (1, 2, 3, 4, 6, 7, 8)},   # dY[L]^T X[L - 1]
    "skip_conn_layer.0.weight": [(DY(5), ACT(4), 0, 256, 0, 256), (DY(5), POSX, 0, 256, 256, 63)],  # dY[5]^T [X[4] ; posx]
    "sigma_fc.0.weight": [(DSR, ACT(7), 3, 1, 0, 256)],                                            # dsr[:, 3:4]^T X[7]
    "color_fc.0.weight": [(DY(9), ACT(8), 0, 128, 0, 256), (DY(9), POSD, 0, 128, 256, 27)],        # dY[9][:, :128]^T [X[8] ; posd]
    "color_fc.2.weight": [(DSR, ACT(9), 0, 3, 0, 128)],                                            # dsr[:, :3]^T X[9][:, :128]
}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """The header as JSON: the table, every plan of the cases below, the scratch layouts."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("dw_products") / "dw_products_dump"
    subprocess.run(["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "nerf-simple_amd", "csrc"),
                    os.path.join(ROOT, "tests", "dw_products_dump.cpp"), "-o", str(exe)], check=True)
    req = [f"plan {form} {bucket} {cus} {P}" for form in FORMS for bucket in (0, 1, 2) for cus in CUS for P in SIZES]
    req += [f"scratch {P}" for P in SCRATCH_SIZES]
    out = subprocess.run([str(exe)], input="\n".join(req) + "\n", check=True, stdout=subprocess.PIPE, text=True).stdout
    return json.loads(out)


def _operand(o):
    return (o["kind"], o["layer"])


def _tensor_of(coff):
    return next(k for k, (off, shape) in M.OFFSETS.items() if off <= coff < off + int(np.prod(shape)))


def test_table_is_the_products_of_the_model(dump):
    rows = dump["products"]
    assert len(rows) == 14 and dump["split"] == M.OFFSETS["skip_conn_layer.0.weight"][0]
    # the stored rectangles tile the weight entries of the flat vector, each entry once, and touch no bias entry
    hits = np.zeros(M.PARAM_COUNT, dtype=np.int64)
    for p in rows:
        idx = p["coff"] + np.arange(p["Mv"])[:, None] * p["ldc"] + np.arange(p["Nv"])[None, :]
        assert idx.min() >= 0 and idx.max() < M.PARAM_COUNT
        np.add.at(hits, idx.reshape(-1), 1)
    for name, (off, shape) in M.OFFSETS.items():
        assert (hits[off:off + int(np.prod(shape))] == (1 if name.endswith(".weight") else 0)).all(), name
    # the bias sums carried by the products: the ten layers whose db is a column sum of dY, each on a product of that layer's
    # whole dY (sigma_fc.0.bias and color_fc.2.bias come from pack_draw_kernel)
    carried = {p["boff"]: p for p in rows if p["boff"] != -1}
    assert len(carried) == sum(p["boff"] != -1 for p in rows)
    assert set(carried) == {M.OFFSETS[M.LAYER_NAMES[L] + ".bias"][0] for L in range(10)}
    for L in range(10):
        off, shape = M.OFFSETS[M.LAYER_NAMES[L] + ".bias"]
        p = carried[off]
        assert _operand(p["a"]) == DY(L) and p["r0"] == 0 and p["Mv"] == shape[0] == M.act_width(L)
    # each row is one operand pair of expected_param_grads, at that tensor's place, and every pair has its row
    want = sorted((name,) + pair for name, pairs in PAIRING.items() for pair in pairs)
    got = []
    for p in rows:
        name = _tensor_of(p["coff"])
        off, shape = M.OFFSETS[name]
        assert p["ldc"] == shape[1] and p["coff"] - off < p["ldc"], name        # starts in the tensor's first row
        got.append((name, _operand(p["a"]), _operand(p["b"]), p["r0"], p["Mv"], p["coff"] - off, p["Nv"]))
    assert sorted(got) == want and len(want) == 14
    # the stored rectangle lies inside what the kernels read, in both forms
    for p in rows:
        for form in FORMS:
            assert p["r0"] + p["Mv"] <= p["a"]["width"][form] and p["Nv"] <= p["b"]["width"][form], (p, form)
    for p in rows:
        for o in (p["a"], p["b"]):
            if o["kind"] in ("DY", "ACT"):
                assert o["width"] == {"bf16": M.act_width(o["layer"]), "e4m3": M.act_width(o["layer"])}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_table_has_the_widths_of_the_model(dump, form):
    """width(a) + width(b) and the head / tail flag of every row: storage_model.PRODUCT_WIDTHS, with the two d_raw rows 32
    instead of 16 features wide in the bf16 form."""
    got = tuple((p["a"]["width"][form] + p["b"]["width"][form], p["coff"] < dump["split"]) for p in dump["products"])
    want = list(S.PRODUCT_WIDTHS)
    if form == "bf16":
        for i in S.DRAW_PRODUCTS:
            want[i] = (want[i][0] + 16, want[i][1])
    assert got == tuple(want) == S.product_widths(FORMS[form]["draw"])
    assert [i for i, p in enumerate(dump["products"]) if p["a"]["kind"] == "DSR"] == list(S.DRAW_PRODUCTS)


def test_plan_equals_the_model(dump):
    """wgs of every (form, bucket, CU count, size) EQUALS storage_model.workgroup_shares -- an independent transcription of the
    arithmetic that predates the header -- and the plan is consistent in itself.  The large sizes run the ``need`` clamp."""
    plans = dump["plans"]
    assert len(plans) == 2 * 3 * len(CUS) * len(SIZES)
    heads = [p["coff"] < dump["split"] for p in dump["products"]]
    seen_need = {form: False for form in FORMS}
    for q in plans:
        form, bucket, cus, P = q["form"], q["bucket"], q["cus"], q["P"]
        f = FORMS[form]
        tag = (form, bucket, cus, P)
        assert q["product"] == [i for i in range(14) if bucket == 0 or heads[i] == (bucket == 2)], tag
        assert q["n"] == len(q["product"]) == len(q["wgs"]) == len(q["wg0"]), tag
        want = S.workgroup_shares(P, bucket, cus, **f)
        assert q["wgs"] == want, tag
        assert q["wg0"] == [sum(want[:i]) for i in range(len(want))] and q["workgroups"] == sum(want), tag
        nslab = (P + f["slab"] - 1) // f["slab"]
        assert all(1 <= w <= nslab for w in q["wgs"]), tag
        if not S.clamp_binds(P, bucket, cus, **f):
            assert sum(q["wgs"]) == cus, tag
        need = (P * 256 * f["bytes_per_feature"] >> 30) + 1
        seen_need[form] |= need > 1 and any(int(s) < need for s in S.ideal_shares(bucket, cus, f["draw"])) and min(q["wgs"]) == need
    assert all(seen_need.values()), seen_need            # the clamp raised a share in both forms
    # ... and without it the cases are not all clamped: 256 CUs with slabs to spare give 256 workgroups
    assert sum(not S.clamp_binds(q["P"], q["bucket"], q["cus"], **FORMS[q["form"]]) for q in plans) > len(plans) // 4


def test_gpu_sizes_hold_the_share_edges_of_the_bf16_form():
    """tests/test_gpu_train_chain.py runs the bf16 kernel at every size where a product's slabs meet its workgroups on the
    256 CUs of the MI355X (the plan there is the model's: test_plan_equals_the_model)."""
    assert set(S.share_edge_sizes(256, **S.BF16_FORM)) <= set(T.INT_SIZES)
    assert set(S.share_edge_sizes()) <= set(S.INT_SIZES)


def test_scratch_layout(dump):
    """posx | posd | dsr, each 256-byte aligned, none overlapping, the total what nerf_amd_param_gradients_scratch_e4m3_bytes
    documents (tests/test_library_cpu.py): per operand ceil(P / 256) tiles of W / 16 chunks of 4 KiB plus 64 exponent bytes."""
    assert [s["P"] for s in dump["scratch"]] == list(SCRATCH_SIZES)
    for s in dump["scratch"]:
        P, tiles = s["P"], (s["P"] + 255) // 256
        size = {W: tiles * (W // 16) * 4096 + tiles * 64 for W in (64, 32, 16)}
        assert s["total"] == sum((n + 255) // 256 * 256 for n in size.values()), P
        if P == 1000:
            assert s["total"] == 4 * (4 + 2 + 1) * 4096 + 3 * 4 * 64
        assert s["px"] == 0 and s["px"] + size[64] <= s["pd"] and s["pd"] + size[32] <= s["ds"] and s["ds"] + size[16] <= s["total"], P
        assert s["px"] % 256 == s["pd"] % 256 == s["ds"] % 256 == 0, P
        offs, total = S.narrow_offsets(P)
        assert (offs, total) == ({64: s["px"], 32: s["pd"], 16: s["ds"]}, s["total"]), P
