"""CPU: transformer-internal dropout -- the host restatement of the mask (Random123 known answers, the site table) and the GoT
constructor / dtype checks.  The GPU side of the same feature is tests/test_gpu_layer_dropout.py."""
import numpy as np
import pytest
import torch

from helpers import O  # noqa: F401  (puts the repository root on sys.path)
import layer_dropout_ref as R


# Philox4x32-10 known-answer vectors of Random123 (kat_vectors: philox4x32 10 rounds)
_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", _KAT)
def test_philox_restatement_matches_random123_known_answers(ctr, key, want):
    got = R.philox4x32_10(np.array([ctr], dtype=np.uint64), key)[0]
    assert [int(v) for v in got] == list(want)


def test_mask_table_counters_and_lanes():
    """The site table: emb-dropout keeps counter word z = 0, site s of layer l uses 0x44000000 | (l << 2) | s, the float4 group index
    is the (x, y) counter and the lane picks the output word."""
    seed, keep = 0x1234_5678_9ABC_DEF0, 0.7
    assert R.site_tag("emb", 3) == 0
    assert R.site_tag(2, 5) == 0x44000000 | (5 << 2) | 2

    def words(i4, tag):
        return R.philox4x32_10(np.array([[i4 & 0xFFFFFFFF, i4 >> 32, tag, 0]], dtype=np.uint64),
                               (seed & 0xFFFFFFFF, seed >> 32))[0]
    thr = lambda w: np.float32(np.uint32(w)) * np.float32(2.0 ** -32) < np.float32(keep)   # noqa: E731
    B, N, D = 2, 5, 8
    m = R.mask(1, 1, (B, N, D), seed, keep).numpy()
    b, t, c = 1, 3, 6
    assert m[b, t, c] == float(thr(words(((b * N + t) * D + c) // 4, R.site_tag(1, 1))[c % 4]))
    H = 3
    a = R.mask(0, 2, (B, H, N, N), seed, keep).numpy()
    b, h, q, k = 1, 2, 4, 4
    i4 = ((b * H + h) * N + q) * ((N + 3) // 4) + k // 4
    assert a[b, h, q, k] == float(thr(words(i4, R.site_tag(0, 2))[k % 4]))
    # different sites / layers draw different bits; the keep fraction is about keep
    big = [R.mask(s, l, (4, 50, 64), seed, keep).numpy() for s, l in ((1, 0), (3, 0), (1, 1), ("emb", 0))]
    for i in range(len(big)):
        assert abs(big[i].mean() - keep) < 0.02
        for j in range(i):
            assert not np.array_equal(big[i], big[j])


def test_masked_restatement_with_all_ones_masks_is_the_oracle():
    """got_forward_masked with all-ones masks (keep = 1) is oracle.got_forward (<= 1e-5)."""
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2, dim_head=32, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 3)
    img, _, _, _ = O.make_inputs(cfg, 2, 3)
    goal = torch.randn(2, cfg.dim, generator=torch.Generator().manual_seed(1))
    ones = {k: (None if v is None else torch.ones_like(v)) for k, v in R.all_masks(cfg, 2, 5, 0.5, 0.9).items()}
    for pool in ("cls", "mean"):
        ref = O.got_forward(params, img, goal, cfg, prefix="", pool=pool)
        got = R.got_forward_masked(params, img, goal, cfg, ones, keep=1.0, emb_keep=1.0, pool=pool)
        assert float((got - ref).abs().max()) <= 1e-5


def _got(dropout, **kw):
    import dgvit_amd
    return dgvit_amd.GoT(image_size=(84, 84), patch_size=(12, 12), num_classes=2, dim=64, depth=2, heads=2, mlp_dim=128, channels=1,
                         dropout=dropout, **kw)


def test_constructor_accepts_transformer_dropout_with_the_same_state_dict():
    a, b = _got(0.1), _got(0.0)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert a.layer_dropout() == pytest.approx(0.1) and b.layer_dropout() == 0.0
    for attn, ff in a.transformer.layers:
        assert attn.fn.dropout.p == pytest.approx(0.1) and attn.fn.to_out[1].p == pytest.approx(0.1)
        assert ff.fn.net[2].p == pytest.approx(0.1) and ff.fn.net[4].p == pytest.approx(0.1)


@pytest.mark.parametrize("p", [1.0, 1.5, -0.1])
def test_constructor_refuses_dropout_outside_zero_one(p):
    with pytest.raises(ValueError, match="dropout"):
        _got(p)


def test_bf16_configuration_refuses_transformer_dropout_in_either_order():
    with pytest.raises(NotImplementedError, match="fp32"):
        _got(0.1).set_compute_dtype(torch.bfloat16)
    m = _got(0.0).set_compute_dtype(torch.bfloat16)      # dropout raised after the dtype: the forward refuses
    for attn, ff in m.transformer.layers:
        attn.fn.dropout.p = attn.fn.to_out[1].p = ff.fn.net[2].p = ff.fn.net[4].p = 0.2
    with pytest.raises(NotImplementedError, match="fp32"):
        m(torch.rand(1, 84, 84), torch.randn(1, 64))
    _got(0.1).set_compute_dtype(torch.float32)           # fp32 stays allowed


def test_got_encoder_checks_the_layer_keep():
    import dgvit_amd
    from dgvit_amd import functional as F_
    m = _got(0.0)
    with pytest.raises(dgvit_amd.DgvitError, match="layer_dropout_keep"):
        F_.got_encoder(torch.rand(1, 84, 84), torch.randn(1, 64), m._cfg, m.param_table(), layer_dropout_keep=0.0)
