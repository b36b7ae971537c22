"""The CQL(H) penalty (dgvit_amd.sac_losses.cql_penalty) restated in torch ops in any dtype on the CPU, value and gradients
in closed form -- the formulas of include/dgvit_hip.h: dgvit_sac_cql_penalty, op by op:

    z[b,m,c] = q_cat[b,m,c] - log_w[b,m]            lse[b,c] = T (mx + log sum_m exp(z / T - mx)),  mx = max_m z / T
    used     = sum_b w_b                            gap_i = sum_{b,c} w_b (lse_i - q_data_i) / (used C)
    loss     = w (gap_1 + gap_2 - 2 tau)            weight_loss = -w (gap_1 + gap_2 - 2 tau)                 tau = 0 outside the Lagrange form
    d q_cat  = w w_b softmax_m(z / T) / (used C)    d q_data = -w w_b / (used C)                             d log_weight = weight_loss

``penalty`` evaluated on float64 tensors is the reference of tests/test_gpu_cql.py, on float32 tensors its yardstick: nothing in either
comes from the device.  tests/test_cql_host.py pins it against torch.logsumexp + autograd."""
import torch

OUTPUTS = ("loss", "gap", "used", "dq1_cat", "dq2_cat", "dq1_data", "dq2_data")
LAGRANGE_OUTPUTS = ("weight_loss", "dlog_weight")

# (B, M, C), T, the scale of the q values
CASES = (((7, 30, 2), 1.0, 1.0), ((7, 30, 2), 0.1, 50.0), ((33, 5, 3), 2.0, 10.0), ((1, 1, 1), 0.7, 3.0), ((257, 3, 16), 1.5, 5.0))


def row_weights(mask, B, dtype):
    if mask is None:
        return torch.ones(B, dtype=dtype)
    return mask.reshape(B).to(dtype)


def penalty(q1_cat, q2_cat, q1_data, q2_data, log_w=None, temperature=1.0, weight=None, log_weight=None, target_gap=None, mask=None):
    """{name: tensor} of OUTPUTS (+ LAGRANGE_OUTPUTS with target_gap) in the dtype of q1_cat"""
    dt = q1_cat.dtype
    B, M, C = q1_cat.shape
    T = torch.tensor(temperature, dtype=dt)
    w = torch.tensor(weight, dtype=dt) if log_weight is None else torch.exp(log_weight.to(dt).reshape(()))
    wb = row_weights(mask, B, dt)
    used = wb.sum()
    inv = 1 / (used * C) if float(used) > 0 else torch.zeros((), dtype=dt)
    out, gaps = {}, []
    for i, (qc, qd) in enumerate(((q1_cat, q1_data), (q2_cat, q2_data)), 1):
        z = qc if log_w is None else qc - log_w.to(dt)[:, :, None]
        zt = z / T
        mx = zt.max(1, keepdim=True).values
        e = torch.exp(zt - mx)
        S = e.sum(1, keepdim=True)
        lse = T * (mx + torch.log(S))[:, 0]
        gaps.append((wb[:, None] * (lse - qd)).sum() * inv)
        coef = w * wb * inv
        out[f"dq{i}_cat"] = coef[:, None, None] * e / S
        out[f"dq{i}_data"] = (-coef)[:, None].expand(B, C).clone()
    excess = gaps[0] + gaps[1] - (2 * torch.tensor(target_gap, dtype=dt) if target_gap is not None else 0)
    if float(used) == 0:
        excess = torch.zeros((), dtype=dt)
    out.update(loss=w * excess, gap=torch.stack(gaps), used=used)
    if target_gap is not None:
        out.update(weight_loss=-w * excess, dlog_weight=(-w * excess).reshape(1))
    return out


def inputs(shape, scale, seed, with_log_w):
    """fp32 inputs of a case (the fp64 reference reads the same numbers)"""
    B, M, C = shape
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    x = dict(q1_cat=scale * n(B, M, C), q2_cat=scale * n(B, M, C), q1_data=scale * n(B, C), q2_data=scale * n(B, C))
    x["log_w"] = (1.5 * n(B, M) - 1.0) if with_log_w else None
    return x


def mixed_mask(B):
    """set explicitly, not drawn: rows 0, 3, 6, ... and the last are used (B = 1: its one row)"""
    m = torch.zeros(B, dtype=torch.bool)
    m[::3] = True
    m[B - 1] = True
    return m
