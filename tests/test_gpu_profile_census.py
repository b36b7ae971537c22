"""GPU: census of the live-profile brackets (csrc/launch.h ProfileScope around every launch, csrc/profile.hip).

bench.py's roofline figures are sums over these brackets, so which launches a bracket encloses, its kind and its work formula are part of
what the library computes.  Each case below runs a fixed set of calls on the product library between dgvit_profile_start and
dgvit_profile_stop at stride 1 and compares the per-kind launch counts and the per-kind work sums of dgvit_profile_totals EXACTLY with a
stored table: the counts are integers and the doubles are the same sums in the same order.

`python tests/test_gpu_profile_census.py` prints the table of the library it runs on.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import O  # noqa: E402

pytestmark = pytest.mark.gpu

GEOM = dict(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=4)     # 49 patches + the goal token


def _bf16(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).cuda().bfloat16()


def _f32(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).cuda()


# ------------------------------------------------------------------------------------------------ kernel-level cases
def _attn_f32(B, H, N, dh, bwd=True):
    def make(amd):
        F = amd.functional
        qkv = _f32(B, N, 3 * H * dh)

        def run():
            out, lse = F.op_attention_fwd(qkv, H, dh)
            if bwd:
                F.op_attention_bwd(qkv, out, torch.ones_like(out), lse, H, dh)
        return run
    return make


def _attn_f32_tiled(B, H, N, dh, nq):
    def make(amd):
        F = amd.functional
        qkv = _f32(B, N, 3 * H * dh)

        def run():
            out, lse = F.op_attention_fwd_tiled(qkv, H, dh, nq=nq)
            dout = torch.zeros_like(out)
            dout[:, :nq] = 1.0
            F.op_attention_bwd_tiled(qkv, out, dout, lse, H, dh, nq=nq)
        return run
    return make


def _attn_bf16(B, H, N, bwd=True):
    def make(amd):
        F = amd.functional
        qkv = _bf16(B, N, 3 * H * 64)

        def run():
            out, lse = F.op_attention_bf16(qkv, H, 64, want_lse=True)
            if bwd:
                F.op_attention_bwd_bf16(qkv, out, torch.ones_like(out), lse, H, 64)
        return run
    return make


def _attn_bf16_tiled(B, H, N):
    def make(amd):
        F = amd.functional
        qkv = _bf16(B, N, 3 * H * 64)

        def run():
            out, lse = F.op_attention_bf16_tiled(qkv, H, 64, want_lse=True)
            F.op_attention_bwd_bf16_tiled(qkv, out, torch.ones_like(out), lse, H, 64)
        return run
    return make


def _gemm_bf16(M, N, K, epilogue):
    def make(amd):
        F = amd.functional
        a, b = _bf16(M, K, seed=1), _bf16(N, K, seed=2)
        bias = _f32(N, seed=3) if epilogue == 0 else None
        aux = _bf16(M, N, seed=4) if epilogue == 3 else None
        return lambda: F.op_gemm_bf16(epilogue, a, b, bias=bias, aux=aux)
    return make


def _wgrad_bf16(T, Mo, Ko):
    def make(amd):
        F = amd.functional
        dy, x = _bf16(T, Mo, seed=1), _bf16(T, Ko, seed=2)
        return lambda: F.op_wgrad_bf16(dy, x)
    return make


# ------------------------------------------------------------------------------------------------ model-level cases
def _policy(amd, dropout):
    cfg = O.GoTConfig(**GEOM)
    m = amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch)
    m.load_state_dict(O.make_params(O.policy_param_spec(cfg), 5), strict=True)
    for mod in m.trans.transformer.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = dropout
    assert m.trans.layer_dropout() == dropout
    m.trans.draw_dropout_seed = lambda: 1234
    return cfg, m.cuda()


def _train_step(dropout):
    def make(amd):
        cfg, m = _policy(amd, dropout)
        m.train()
        from dgvit_amd.optim import FlatAdam
        opt = FlatAdam([m], lr=1e-3)
        img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, 4, 5))

        def run():
            opt.zero_grad()
            mean, log_std = m([img, pstate])
            ((mean ** 2).mean() + (log_std ** 2).mean()).backward()
            opt.step()
        return run
    return make


def _nograd_forward(batch):
    def make(amd):
        cfg, m = _policy(amd, 0.0)
        m.eval()
        img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, batch, 5))

        def run():
            with torch.no_grad():
                m([img, pstate])
        return run
    return make


def _got_bf16_step(batch):
    def make(amd):
        cfg = O.GoTConfig(**GEOM)
        m = amd.GoT(image_size=cfg.image, patch_size=cfg.patch, num_classes=cfg.num_classes, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads,
                    mlp_dim=cfg.mlp_dim, channels=1, dim_head=cfg.dim_head)
        m.load_state_dict(O.make_params(O.got_param_spec(cfg, prefix=""), 7), strict=True)
        m = m.cuda().eval().set_compute_dtype(torch.bfloat16)
        img, _, _, _ = O.make_inputs(cfg, batch, 7)
        img, goal = img.cuda(), _f32(batch, cfg.dim, seed=8)

        def run():
            for q in m.parameters():
                q.grad = None
            g = goal.clone().requires_grad_(True)
            m(img, g).sum().backward()
        return run
    return make


CASES = {
    "attn_f32_n20": _attn_f32(2, 2, 20, 64),                          # one tile
    "attn_f32_n40": _attn_f32(2, 2, 40, 64),                          # two tiles; single-pass backward
    "attn_f32_n100": _attn_f32(2, 2, 100, 64),                        # four waves
    "attn_f32_pipelined_fwd": _attn_f32(256, 8, 40, 32, bwd=False),   # B * H >= 2048: the pipelined forward
    "attn_f32_tiled_n130": _attn_f32_tiled(1, 2, 130, 64, 130),
    "attn_f32_tiled_n130_nq1": _attn_f32_tiled(1, 2, 130, 64, 1),
    "attn_bf16_n40": _attn_bf16(1, 2, 40),                            # four-wave kernel
    "attn_bf16_n200": _attn_bf16(1, 2, 200),                          # eight waves
    "attn_bf16_n257": _attn_bf16(1, 2, 257),                          # above 64 KB of LDS, nine waves
    "attn_bf16_stream_n160_fwd": _attn_bf16(64, 8, 160, bwd=False),   # persistent stream kernel (>= 512 items)
    "attn_bf16_stream_n257_fwd": _attn_bf16(64, 8, 257, bwd=False),   # 288-row persistent kernel
    "attn_bf16_tiled_n300": _attn_bf16_tiled(1, 2, 300),
    "gemm_bf16_100x64x64": _gemm_bf16(100, 64, 64, 0),                # 64-tile
    "gemm_bf16_2048x1024x64": _gemm_bf16(2048, 1024, 64, 0),          # 128-tile
    "gemm_bf16_8192x4096x64_bf16": _gemm_bf16(8192, 4096, 64, 0),     # stream kernel
    "gemm_bf16_8192x4096x64_dgelu": _gemm_bf16(8192, 4096, 64, 3),    # ring kernel: the stream kernel does not take this epilogue
    "wgrad_bf16_t4096_256x256": _wgrad_bf16(4096, 256, 256),          # TN, split-K, slab reduction
    "train_step": _train_step(0.0),                                   # last-block fold, fused heads
    "train_step_layer_dropout": _train_step(0.1),                     # general attention kernels, the unfolded last block
    "nograd_forward_b1": _nograd_forward(1),                          # block path
    "nograd_forward_b80": _nograd_forward(80),                        # GEMM schedule, one-query attention
    "got_bf16_step_b2": _got_bf16_step(2),
}

# name -> (launches per kind, work per kind), kinds 0 GEMM, 1 attention forward, 2 attention backward, 3 other.
# Captured with `python tests/test_gpu_profile_census.py` on commit 9531c3a (the parent of the commit that introduced csrc/launch.h).
TABLE = {
    "attn_f32_n20": ([0, 1, 1, 0], [0.0, 409600.0, 819200.0, 0.0]),
    "attn_f32_n40": ([0, 1, 1, 0], [0.0, 1638400.0, 3276800.0, 0.0]),
    "attn_f32_n100": ([0, 1, 1, 0], [0.0, 10240000.0, 20480000.0, 0.0]),
    "attn_f32_pipelined_fwd": ([0, 1, 0, 0], [0.0, 419430400.0, 0.0, 0.0]),
    "attn_f32_tiled_n130": ([0, 1, 1, 0], [0.0, 8652800.0, 17305600.0, 0.0]),
    "attn_f32_tiled_n130_nq1": ([0, 1, 1, 0], [0.0, 66560.0, 133120.0, 0.0]),
    "attn_bf16_n40": ([0, 1, 1, 0], [0.0, 819200.0, 2048000.0, 0.0]),
    "attn_bf16_n200": ([0, 1, 1, 0], [0.0, 20480000.0, 51200000.0, 0.0]),
    "attn_bf16_n257": ([0, 1, 1, 0], [0.0, 33817088.0, 84542720.0, 0.0]),
    "attn_bf16_stream_n160_fwd": ([0, 1, 0, 0], [0.0, 3355443200.0, 0.0, 0.0]),
    "attn_bf16_stream_n257_fwd": ([0, 1, 0, 0], [0.0, 8657174528.0, 0.0, 0.0]),
    "attn_bf16_tiled_n300": ([0, 1, 1, 0], [0.0, 46080000.0, 115200000.0, 0.0]),
    "gemm_bf16_100x64x64": ([1, 0, 0, 0], [819200.0, 0.0, 0.0, 0.0]),
    "gemm_bf16_2048x1024x64": ([1, 0, 0, 0], [268435456.0, 0.0, 0.0, 0.0]),
    "gemm_bf16_8192x4096x64_bf16": ([1, 0, 0, 0], [4294967296.0, 0.0, 0.0, 0.0]),
    "gemm_bf16_8192x4096x64_dgelu": ([1, 0, 0, 0], [4294967296.0, 0.0, 0.0, 0.0]),
    "wgrad_bf16_t4096_256x256": ([1, 0, 0, 3], [536870912.0, 0.0, 0.0, 0.0]),
    "train_step": ([28, 2, 2, 15], [407521280.0, 10444800.0, 20889600.0, 786432.0]),
    "train_step_layer_dropout": ([31, 2, 2, 10], [446842880.0, 10444800.0, 20889600.0, 0.0]),
    "nograd_forward_b1": ([2, 0, 0, 5], [903424.0, 0.0, 0.0, 0.0]),
    "nograd_forward_b80": ([11, 2, 0, 1], [3003043840.0, 208896000.0, 0.0, 0.0]),
    "got_bf16_step_b2": ([26, 2, 2, 28], [396828672.0, 10240000.0, 25600000.0, 0.0]),
}


def census(amd, make):
    """(launches per kind, work_all per kind) of one run of the case, after one unrecorded run (lazy allocations, packed weights)"""
    from dgvit_amd import _lib
    lib = amd.load_library()
    run = make(amd)
    run()
    torch.cuda.synchronize()
    kinds = _lib.PROFILE_KINDS
    assert lib.dgvit_profile_sampling(1) == 0
    try:
        assert lib.dgvit_profile_start(8192) == 0
        run()
        torch.cuda.synchronize()
        ms, work, cnt = (ctypes.c_double * kinds)(), (ctypes.c_double * kinds)(), (ctypes.c_longlong * kinds)()
        assert lib.dgvit_profile_stop(ms, work, cnt) == 0, lib.dgvit_last_error()
        work_all, cnt_all = (ctypes.c_double * kinds)(), (ctypes.c_longlong * kinds)()
        assert lib.dgvit_profile_totals(work_all, cnt_all) == 0
    finally:
        lib.dgvit_profile_sampling(1)      # (1 is the library's default stride; there is no getter to save and restore another)
    assert list(cnt) == list(cnt_all) and list(work) == list(work_all)      # stride 1: every launch seen was timed
    return list(cnt_all), list(work_all)


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


@pytest.mark.parametrize("case", list(CASES))
def test_profile_census(amd, case):
    got = census(amd, CASES[case])
    print(f"{case}: {got}")
    assert got == TABLE[case]


if __name__ == "__main__":
    import dgvit_amd
    dgvit_amd.load_library()
    print("TABLE = {")
    for name, make in CASES.items():
        cnt, work = census(dgvit_amd, make)
        print(f"    {name!r}: ({cnt!r}, {work!r}),", flush=True)
    print("}")
