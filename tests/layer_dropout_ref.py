"""Host restatement of the encoder's dropout masks and an fp64 model of GoT.forward with them (shared by the layer-dropout tests).

* ``philox4x32_10``: Philox4x32-10 (Random123) in numpy uint64 arithmetic, vectorised over counters.
* ``mask(site, layer, shape, seed, keep)``: the {0, 1} keep mask of one dropout site, following the table in include/dgvit_hip.h
  (dgvit_got_forward_v2) -- independent of the kernels, so it pins the counter scheme.
* ``got_forward_masked``: GoT.forward (GoalFormer.py:156-171) in fp64 with explicit masks at all five sites.
"""
import numpy as np
import torch

from oracle import dgvit_oracle as O

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)

SITE_EMB, SITE_ATTN, SITE_OUT, SITE_HIDDEN, SITE_FF = "emb", 0, 1, 2, 3


def philox4x32_10(ctr, key):
    """ctr: (..., 4) uint32-valued, key: (2,) -> (..., 4) uint64 holding the four output words."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _U32
        hi1, lo1 = p1 >> np.uint64(32), p1 & _U32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(_W0)) & _U32
        k1 = (k1 + np.uint64(_W1)) & _U32
    return np.stack(c, axis=-1)


def site_tag(site, layer):
    """The third counter word: 0 for emb-dropout, 0x44000000 | (layer << 2) | site for the transformer sites."""
    return 0 if site == SITE_EMB else 0x44000000 | (layer << 2) | site


def _keep_words(i4, tag, seed, keep):
    """(..., 4) bool: the words of the Philox blocks at float4 indices i4 below keep (r * 2^-32 < keep in fp32, as dropout4)."""
    i4 = np.asarray(i4, dtype=np.uint64)
    ctr = np.stack([i4 & _U32, i4 >> np.uint64(32), np.full_like(i4, tag), np.zeros_like(i4)], axis=-1)
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return r.astype(np.uint32).astype(np.float32) * np.float32(2.0 ** -32) < np.float32(keep)


def mask(site, layer, shape, seed, keep, frames=None):
    """{0, 1} float64 mask of one site (``frames``: only these frames b of the batch, in that order; shape keeps the full B).
    emb / 1 / 2 / 3: shape (B, N, W), element (b, t, c) -> float4 group ((b*N + t)*W + c) // 4, lane c % 4
    0 (attention probabilities): shape (B, H, N, N), element (b, h, q, k) -> group ((b*H + h)*N + q)*ceil(N/4) + k // 4, lane k % 4"""
    if site == SITE_ATTN:
        B, H, N, N2 = shape
        assert N == N2
        n4 = (N + 3) // 4
        fr = np.arange(B) if frames is None else np.asarray(frames)
        rows = np.arange(B * H * N, dtype=np.uint64).reshape(B, H, N, 1)[fr]
        i4 = rows * np.uint64(n4) + np.arange(n4, dtype=np.uint64)
        m = _keep_words(i4, site_tag(site, layer), seed, keep).reshape(len(fr), H, N, 4 * n4)[..., :N]
    else:
        B, N, W = shape
        assert W % 4 == 0
        fr = np.arange(B) if frames is None else np.asarray(frames)
        i4 = (fr.astype(np.uint64).reshape(-1, 1, 1) * np.uint64(N * W // 4) + np.arange(N * W // 4, dtype=np.uint64).reshape(1, N, W // 4))
        m = _keep_words(i4, site_tag(site, layer), seed, keep).reshape(len(fr), N, W)
    return torch.from_numpy(m.astype(np.float64))


def all_masks(cfg, B, seed, keep, emb_keep, frames=None):
    """Every mask one train-mode forward draws: {"emb": ..., (layer, site): ...}; no site 1 without an output projection."""
    N, D, H, M = cfg.tokens, cfg.dim, cfg.heads, cfg.mlp_dim
    out = {SITE_EMB: mask(SITE_EMB, 0, (B, N, D), seed, emb_keep, frames) if emb_keep < 1 else None}
    for l in range(cfg.depth):
        out[(l, SITE_ATTN)] = mask(SITE_ATTN, l, (B, H, N, N), seed, keep, frames)
        out[(l, SITE_OUT)] = mask(SITE_OUT, l, (B, N, D), seed, keep, frames) if cfg.project_out else None
        out[(l, SITE_HIDDEN)] = mask(SITE_HIDDEN, l, (B, N, M), seed, keep, frames)
        out[(l, SITE_FF)] = mask(SITE_FF, l, (B, N, D), seed, keep, frames)
    return out


def _drop(x, masks, key, keep):
    m = masks.get(key) if masks else None
    return x if m is None else x * m.to(x.dtype) / keep


def got_forward_masked(p, img, goal, cfg, masks=None, keep=1.0, emb_keep=1.0, pool="cls"):
    """GoT.forward with train-mode dropout at the five sites; p keyed without prefix, computed in the dtype of its tensors."""
    lin = O.linear
    x = lin(O.patchify(img, cfg).to(goal.dtype), p["to_patch_embedding.1.weight"], p["to_patch_embedding.1.bias"])
    x = torch.cat([goal.unsqueeze(1), x], dim=1) + p["pos_embedding"][:, :cfg.tokens]
    x = _drop(x, masks, SITE_EMB, emb_keep)
    B, N, I, H, dh = x.shape[0], cfg.tokens, cfg.inner, cfg.heads, cfg.dim_head
    for l in range(cfg.depth):
        lp = f"transformer.layers.{l}."
        h = O.layer_norm(x, p[lp + "0.norm.weight"], p[lp + "0.norm.bias"])
        qkv = lin(h, p[lp + "0.fn.to_qkv.weight"])
        q, k, v = (qkv[..., j * I:(j + 1) * I].reshape(B, N, H, dh).permute(0, 2, 1, 3) for j in range(3))
        attn = torch.softmax((q @ k.transpose(-1, -2)) * dh ** -0.5, dim=-1)
        attn = _drop(attn, masks, (l, SITE_ATTN), keep)                                      # GoalFormer.py:78
        a = (attn @ v).permute(0, 2, 1, 3).reshape(B, N, I)
        if cfg.project_out:
            a = _drop(lin(a, p[lp + "0.fn.to_out.0.weight"], p[lp + "0.fn.to_out.0.bias"]), masks, (l, SITE_OUT), keep)   # :68
        x = a + x
        h = O.layer_norm(x, p[lp + "1.norm.weight"], p[lp + "1.norm.bias"])
        h = _drop(O.gelu_exact(lin(h, p[lp + "1.fn.net.0.weight"], p[lp + "1.fn.net.0.bias"])), masks, (l, SITE_HIDDEN), keep)  # :47
        x = _drop(lin(h, p[lp + "1.fn.net.3.weight"], p[lp + "1.fn.net.3.bias"]), masks, (l, SITE_FF), keep) + x               # :49
    pooled = x.mean(dim=1) if pool == "mean" else x[:, 0]
    return O.rms_norm(pooled, p["layer_norm.g"])


def build_got(amd, cfg, dropout, pool="cls", emb_dropout=0.1):
    return amd.GoT(image_size=cfg.image, patch_size=cfg.patch, num_classes=cfg.num_classes, dim=cfg.dim, depth=cfg.depth,
                   heads=cfg.heads, mlp_dim=cfg.mlp_dim, channels=1, dim_head=cfg.dim_head, pool=pool, dropout=dropout,
                   emb_dropout=emb_dropout)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-12))


__all__ = ["philox4x32_10", "mask", "all_masks", "got_forward_masked", "build_got", "rel_err", "site_tag"]
