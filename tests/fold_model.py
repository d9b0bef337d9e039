"""CPU emulation of the FOLDED fp16 inference numerics (test infrastructure; uses the oracle and tests/error_model.py).

The fp16 inference kernels do not form h9 = layers_2(h8): the packer pre-multiplies Wf = Wc[:, :256] W2 and
bf = bc + Wc[:, :256] b2 in fp32 (csrc/nerf_layout.h, folded view) and the colour layer computes
relu([Wf | Wc[:, 256:]] [h8 ; gamma(d)] + bf).  What is rounded to fp16 is therefore Wf and h8 instead of W2, h8, Wc and
h9; everything else is tests/studies/precision_study.py's emulation unchanged (operands rounded, fp32 products and sums,
fp32 bias).
"""
import torch
import torch.nn.functional as F

import error_model


def folded_weights(sd, dtype=torch.float32):
    """(Wf [128,256], bf [128]) formed in `dtype`."""
    Wc, bc = sd["color_fc.0.weight"].to(dtype), sd["color_fc.0.bias"].to(dtype)
    W2, b2 = sd["layers_2.weight"].to(dtype), sd["layers_2.bias"].to(dtype)
    return Wc[:, :256] @ W2, bc + Wc[:, :256] @ b2


def forward(sd, v, kind="fp16"):
    """Nerf.forward with the folded kernels' numerics: [P,6] -> [P,4]."""
    import nerf_oracle as O
    S = error_model.study()
    with torch.no_grad():
        x, d = O.positional_encoder(v)
        h = x
        for i in (0, 2, 4, 6, 8):
            h = F.relu(S.lin(h, sd[f"layers_0.{i}.weight"], sd[f"layers_0.{i}.bias"], kind))
        h = F.relu(S.lin(torch.cat([h, x], 1), sd["skip_conn_layer.0.weight"], sd["skip_conn_layer.0.bias"], kind))
        for i in (0, 2):
            h = F.relu(S.lin(h, sd[f"layers_1.{i}.weight"], sd[f"layers_1.{i}.bias"], kind))
        sigma = S.lin(h, sd["sigma_fc.0.weight"], sd["sigma_fc.0.bias"], kind)
        Wf, bf = folded_weights(sd)
        c = F.relu(S.lin(torch.cat([h, d], 1), torch.cat([Wf, sd["color_fc.0.weight"][:, 256:]], 1), bf, kind))
        rgb = S.lin(c, sd["color_fc.2.weight"], sd["color_fc.2.bias"], kind)
        return torch.cat([rgb, sigma], 1)


def render(sd, rays, u, kind="fp16"):
    """render_nerf with the folded numerics (fp32 sampling and compositing, as in the kernels): the 5-tuple."""
    import nerf_oracle as O
    with torch.no_grad():
        ts = O.sample_ts(u)
        q, dn = O.query_points(rays, ts)
        out = forward(sd, q, kind).reshape(rays.shape[0], u.shape[1], 4)
        return O.volume_render(out, ts, dn)
