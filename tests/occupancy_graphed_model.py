"""numpy restatement of the graphed masked training step's capacity semantics (include/nerf_amd.h, "graphed masked
training step"; csrc/occupancy_graph.hip; training.GraphedMaskedTrainStep), after tests/occupancy_model.py and
tests/occupancy_train_model.py.  Test infrastructure; nothing here is fitted to what the GPU showed.

A graphed masked step is captured for a fixed point capacity C, 1 <= C <= B N, and every network kernel runs on exactly C
points on every replay.  With ``live`` [B, N] the grid's verdict on the batch's samples and P' = live.sum():

  kept samples: sample i of ray b is KEPT iff it is live and its global rank r = offsets[b] + (live samples of the ray
      before i) is < C: ``mask_C``.  Its exclusive scan is ``offsets_C`` = min(offsets, C).  The step is, by definition, the
      masked step of occupancy_train_model with mask_C in place of the mask: with P' <= C nothing changes, with P' > C the
      tail of the live samples in ray-major order is dead, (0, 0, 0, -inf), contributing nothing and receiving nothing.
  surplus rows r in [min(P', C), C): pts[r] = PAD_POINT, d_raw_live[r] = 0.
  counts = (P', min(P', C)).
"""
import numpy as np

import occupancy_model as M

PAD_POINT = (0.0, 0.0, 0.0, 0.0, 0.0, -1.0)           # NERF_AMD_OCCUPANCY_PAD_POINT


def mask_C(live, C):
    """live [B, N] bool -> the kept samples [B, N] bool: the first C live samples in ray-major order"""
    live = np.asarray(live, dtype=bool)
    rank = np.cumsum(live.reshape(-1), dtype=np.int64) - 1          # global rank of a live sample, ray-major
    return (live.reshape(-1) & (rank < int(C))).reshape(live.shape)


def mask_C_loop(live, C):
    """the definition spelled out: offsets[b] + (live samples of the ray before i) < C, sample by sample"""
    live = np.asarray(live, dtype=bool)
    off = M.offsets(live)
    out = np.zeros_like(live)
    for b in range(live.shape[0]):
        before = 0
        for i in range(live.shape[1]):
            if live[b, i]:
                out[b, i] = int(off[b]) + before < int(C)
                before += 1
    return out


def offsets_C(live, C):
    return np.minimum(M.offsets(live), int(C)).astype(np.int64)


def counts(live, C):
    total = int(np.asarray(live, dtype=bool).sum())
    return total, min(total, int(C))


def capped_points(points_live, C):
    """points_live [P', 6] (the rows of the uncapped emit) -> pts [C, 6]"""
    points_live = np.asarray(points_live, dtype=np.float32).reshape(-1, 6)
    out = np.tile(np.asarray(PAD_POINT, dtype=np.float32), (int(C), 1))
    k = min(points_live.shape[0], int(C))
    out[:k] = points_live[:k]
    return out


def capacities(total, B, N):
    """the capacities the tests derive from a live count P' (never typed in), clipped to [1, B N], duplicates dropped:
    P', P' + 1, the next multiple of 256, P' - 1, ceil(P' / 2) (cuts inside a ray), 1, B N"""
    want = [total, total + 1, -(-(total + 1) // 256) * 256, total - 1, -(-total // 2), 1, B * N]
    out = []
    for c in want:
        c = min(max(int(c), 1), B * N)
        if c not in out:
            out.append(c)
    return out
