"""CPU (no GPU): the bf16 encoder's size queries for patch areas that are not multiples of 8 (14x14, 7x7, 3x5: ViT-S/B/L at /14).

The rows of the bf16 patch operands (the patches in the workspace, the patch weight in the arena) are padded to ldp = pd rounded up to 8
elements; nothing else depends on pd.  So a configuration and its "twin" -- the same patch grid, widths and batch, with a patch whose
area IS a multiple of 8 -- differ in those two slots only, which pins the growth exactly without restating the layout here.  For
patch areas that are multiples of 8 the queries must return what the build before this change returned (constants below)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


def _cfg(image, patch, dim, depth, heads, mlp, dim_head=64):
    from dgvit_amd._lib import dgvit_config
    return dgvit_config(image[0], image[1], patch[0], patch[1], dim, depth, heads, dim_head, mlp)


def _queries(lib, cfg, B):
    r = ctypes.byref(cfg)
    return (lib.dgvit_got_bf16_weight_elems(r), lib.dgvit_got_bf16_workspace_bytes(r, B, 0), lib.dgvit_got_bf16_workspace_bytes(r, B, 1),
            lib.dgvit_got_bf16_backward_scratch_bytes(r, B))


def up8(n):
    return (n + 7) & ~7


def al4(n):
    return (n + 3) & ~3


def al256(n):
    return (n + 255) & ~255


# (image, patch, twin image, twin patch, dim, depth, heads, mlp, batch): the twin has the same patch grid and pd % 8 == 0
NEW_SHAPES = {
    "vits14_224": ((224, 224), (14, 14), (256, 256), (16, 16), 384, 12, 6, 1536, 8),
    "vitb14_224": ((224, 224), (14, 14), (256, 256), (16, 16), 768, 12, 12, 3072, 8),
    "vitl14_224": ((224, 224), (14, 14), (256, 256), (16, 16), 1024, 24, 16, 4096, 2),
    "84p7": ((84, 84), (7, 7), (96, 96), (8, 8), 64, 2, 2, 128, 3),
    "30x50p3x5": ((30, 50), (3, 5), (40, 80), (4, 8), 64, 2, 2, 128, 5),
}


@pytest.mark.parametrize("name", list(NEW_SHAPES))
def test_size_queries_accept_patch_areas_off_the_multiples_of_8(lib, name):
    image, patch, timage, tpatch, dim, depth, heads, mlp, B = NEW_SHAPES[name]
    pd, tpd = patch[0] * patch[1], tpatch[0] * tpatch[1]
    ldp = up8(pd)
    assert pd % 8 and tpd % 8 == 0
    P = (image[0] // patch[0]) * (image[1] // patch[1])
    assert P == (timage[0] // tpatch[0]) * (timage[1] // tpatch[1])
    got = _queries(lib, _cfg(image, patch, dim, depth, heads, mlp), B)
    assert all(v > 0 for v in got), (got, lib.dgvit_last_error())
    twin = _queries(lib, _cfg(timage, tpatch, dim, depth, heads, mlp), B)
    # arena: everything but the patch weight is the twin's; the patch weight takes al4(D * ldp) -- (ldp - pd) * D elements more than
    # the unpadded al4(D * pd)
    rest = twin[0] - al4(dim * tpd)
    assert got[0] == rest + al4(dim * ldp)
    assert got[0] - (rest + al4(dim * pd)) == (ldp - pd) * dim
    # workspace (no-grad and save-for-backward layouts): the patches slot takes B * P * ldp * 2 bytes through the 256-byte rounding
    for i in (1, 2):
        rest = twin[i] - al256(B * P * tpd * 2)
        assert got[i] == rest + al256(B * P * ldp * 2)
        grown = got[i] - (rest + al256(B * P * pd * 2))              # over the unpadded layout
        assert abs(grown - B * P * (ldp - pd) * 2) < 256 and grown % 256 == 0


# pd % 8 == 0: (weight elements, workspace bytes no-grad, workspace bytes save-for-backward, backward scratch bytes) as the library
# built from the commit before this change returned them (printed by its size queries on the host; no GPU is involved)
PARENT = [
    ("c5_b440", ((224, 224), (16, 16), 768, 12, 12, 3072), 440, (170065920, 2179915008, 29536132096, 2035080448)),
    ("vitb16_256_b440", ((256, 256), (16, 16), 768, 12, 12, 3072), 440, (170065920, 2843505408, 38531556352, 2631136000)),
    ("128x160p8x10", ((128, 160), (8, 10), 128, 2, 2, 256), 5, (534528, 4823296, 11127040, 5287168)),
    ("84p12_d64", ((84, 84), (12, 12), 64, 2, 4, 128), 4, (336896, 726528, 1531648, 793344)),
    ("84p12_shipped", ((84, 84), (12, 12), 256, 6, 4, 2048), 512, (15765504, 270303232, 2122924032, 322093056)),
    ("vits16_224", ((224, 224), (16, 16), 384, 12, 6, 1536), 32, (42565632, 80875264, 1076257792, 106598144)),
    ("32p8", ((32, 32), (8, 8), 64, 1, 2, 64), 1, (86016, 39936, 49920, 58368)),
    ("12x16p2x4", ((12, 16), (2, 4), 64, 2, 2, 128), 3, (197120, 175872, 401920, 168960)),
]


@pytest.mark.parametrize("name,shape,B,want", PARENT, ids=[c[0] for c in PARENT])
def test_size_queries_unchanged_for_patch_areas_that_are_multiples_of_8(lib, name, shape, B, want):
    assert (shape[1][0] * shape[1][1]) % 8 == 0
    assert _queries(lib, _cfg(*shape), B) == want


def test_other_bf16_refusals_stand_with_an_odd_patch(lib):
    """7x7 patches no longer refuse; what else the bf16 path refuses, it still refuses (and says which)"""
    r = ctypes.byref
    bad = _cfg((84, 84), (7, 7), 100, 2, 2, 2048)                  # dim not a multiple of 8
    assert lib.dgvit_got_bf16_weight_elems(r(bad)) < 0
    msg = lib.dgvit_last_error()
    assert b"dim" in msg and b"patch" not in msg, msg
    bad = _cfg((84, 84), (12, 12), 100, 2, 2, 2048)
    assert lib.dgvit_got_bf16_weight_elems(r(bad)) < 0 and b"dim" in lib.dgvit_last_error()
    bad = _cfg((84, 84), (7, 7), 64, 2, 2, 100)                    # mlp_dim not a multiple of 8
    assert lib.dgvit_got_bf16_workspace_bytes(r(bad), 2, 0) < 0 and b"mlp_dim" in lib.dgvit_last_error()
    bad = _cfg((84, 84), (7, 7), 256, 2, 8, 2048, dim_head=32)     # dim_head 32: fp32 path only
    assert lib.dgvit_got_bf16_workspace_bytes(r(bad), 4, 0) < 0 and b"dim_head" in lib.dgvit_last_error()
    assert lib.dgvit_got_bf16_backward_scratch_bytes(r(bad), 4) < 0 and b"dim_head" in lib.dgvit_last_error()
    bad = _cfg((84, 84), (7, 7), 64, 2, 1, 128, dim_head=64)       # heads == 1, dim_head == dim: attention without to_out
    assert lib.dgvit_got_bf16_weight_elems(r(bad)) < 0 and b"output projection" in lib.dgvit_last_error()
    ok = _cfg((84, 84), (7, 7), 64, 2, 2, 128)
    assert lib.dgvit_got_bf16_weight_elems(r(ok)) > 0


def test_header_no_longer_asks_for_patch_pixels_in_multiples_of_8():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "dgvit_hip.h")).read()
    assert "patch pixels % 8" not in text
