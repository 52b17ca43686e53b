"""Deterministic mode without a GPU: the "deterministic" option of bvc_set_option, the Python switches (bvc.use_deterministic_algorithms
and torch's own flag, ORed at every library call), and the kernel instantiations the GEMM launcher names for the products whose
default kernels accumulate by f32 atomics (bvc_op_gemm_kernel launches nothing)."""
import ctypes

import pytest
import torch


def _desc(L, M, N, K, split=1, rowsum=False):
    d = L.GemmDesc()
    d.A, d.B, d.C = 4096, 8192, 4096          # never dereferenced: nothing is launched
    d.M, d.N, d.K = M, N, K
    d.alpha, d.epi, d.split_k, d.ldc = 1.0, 0, split, N
    d.a_bytes, d.b_bytes = M * K * 2, N * K * 2
    d.lda, d.ldb = M, N                        # TN: dW[M, N] = dY^T X over K tokens
    d.rowsum = 4096 if rowsum else None
    return d


def _name(L, descs, layout, tile=-1):
    arr = (L.GemmDesc * len(descs))(*descs)
    buf = ctypes.create_string_buffer(160)
    L.check(L.lib().bvc_op_gemm_kernel(arr, len(descs), layout, tile, -1, buf, 160), "bvc_op_gemm_kernel")
    return buf.value.decode()


def _dw_group(L, M, D, I):
    return [_desc(L, D, I, M, rowsum=True), _desc(L, I, D, M, rowsum=True), _desc(L, D, D, M, rowsum=True),
            _desc(L, 3 * D, D, M, rowsum=True)]


def _plan(L, descs):
    arr = (L.GemmDesc * len(descs))(*descs)
    tile = L.lib().bvc_op_gemm_plan_dw(arr, len(descs))
    return tile, list(arr)


def _is_det(name):
    return name.startswith("bvc::gemm_det_kernel<") or (name.startswith("bvc::gemm8_kernel<") and name.endswith(", 6>"))


@pytest.fixture
def L(bvc):
    lib = bvc._lib
    old_g8 = lib.set_option("gemm8", 0)
    old_flag, old_torch = bvc.are_deterministic_algorithms_enabled(), torch.are_deterministic_algorithms_enabled()
    try:
        yield lib
    finally:
        torch.use_deterministic_algorithms(old_torch)
        bvc.use_deterministic_algorithms(old_flag)
        lib.set_option("deterministic", 0)
        lib.set_option("gemm8", old_g8)


def test_option_defaults_round_trips_and_rejects_other_values(L):
    lib = L.lib()
    assert lib.bvc_get_option(b"deterministic") == 0
    assert lib.bvc_set_option(b"deterministic", 1) == 0 and lib.bvc_get_option(b"deterministic") == 1
    assert lib.bvc_set_option(b"deterministic", 0) == 0 and lib.bvc_get_option(b"deterministic") == 0
    for bad in (2, -1):
        assert lib.bvc_set_option(b"deterministic", bad) == -1       # BVC_ERR_INVALID
        assert lib.bvc_get_option(b"deterministic") == 0
    assert "deterministic" in L.set_option.__doc__


def test_python_and_torch_flags_switch_the_effective_mode(L, bvc):
    probe = [_desc(L, 768, 3072, 2560, split=4)]
    default = _name(L, probe, 2, 0)
    assert default == "bvc::gemm_kernel<128, 128, true, true, 2, 2, true>"
    assert not bvc.are_deterministic_algorithms_enabled()
    bvc.use_deterministic_algorithms(True)
    assert bvc.are_deterministic_algorithms_enabled()
    assert _name(L, probe, 2, 0) == "bvc::gemm_det_kernel<128, 128, true, true>"
    assert L.lib().bvc_get_option(b"deterministic") == 1
    bvc.use_deterministic_algorithms(False)
    assert _name(L, probe, 2, 0) == default
    torch.use_deterministic_algorithms(True, warn_only=True)
    assert _name(L, probe, 2, 0) == "bvc::gemm_det_kernel<128, 128, true, true>"
    torch.use_deterministic_algorithms(False)
    assert _name(L, probe, 2, 0) == default
    assert L.lib().bvc_get_option(b"deterministic") == 0


@pytest.mark.parametrize("clips", [16, 64, 256])
def test_videomae_base_weight_gradient_groups_name_deterministic_kernels(L, bvc, clips):
    # encoder layer (160 visible tokens per clip, 768 / 3072) and decoder layer (1568 tokens per clip, 384 / 1536), plus the plans a
    # forced gemm8 gives them (tile config 10 / 12 / 13 included)
    groups = [_dw_group(L, clips * 160, 768, 3072), _dw_group(L, clips * 1568, 384, 1536), _dw_group(L, clips * 160, 1024, 4096)]
    seen = set()
    for g8 in (0, 1):
        L.set_option("gemm8", g8)
        for group in groups:
            bvc.use_deterministic_algorithms(False)
            tile, planned = _plan(L, group)
            default = _name(L, planned, 2, tile)
            bvc.use_deterministic_algorithms(True)
            tile_d, planned_d = _plan(L, group)
            assert tile_d == tile and [d.split_k for d in planned_d] == [d.split_k for d in planned], "plans do not depend on the mode"
            det = _name(L, planned_d, 2, tile)
            assert _is_det(det) and det != default, (clips, tile, det)
            assert "atomic" not in det
            seen.add((tile, planned[0].split_k > 1))
            bvc.use_deterministic_algorithms(False)
            assert _name(L, planned, 2, tile) == default
    assert any(split for _, split in seen), seen


def test_config_13_and_split_groups_without_bias_gradients(L, bvc):
    group = [_desc(L, 1024, 4096, 25600), _desc(L, 4096, 1024, 25600)]
    assert _name(L, group, 2, 13) == "bvc::gemm8_kernel<256, 256, true, true, 2>"
    bvc.use_deterministic_algorithms(True)
    assert _name(L, group, 2, 13) == "bvc::gemm8_kernel<256, 256, true, true, 6>"
    split = [_desc(L, 384, 1536, 40000, split=7)]
    assert _name(L, split, 2, 12) == "bvc::gemm8_kernel<128, 384, true, true, 6>"
    # unsplit, non-accumulating products without a bias gradient have no atomics: they keep the default kernels
    plain = [_desc(L, 384, 1536, 40000)]
    bvc.use_deterministic_algorithms(False)
    want = _name(L, plain, 2, 12)
    bvc.use_deterministic_algorithms(True)
    assert _name(L, plain, 2, 12) == want


def test_simclr_head_bias_gradient_products(L, bvc):
    # SimCLR projection head backward (simclr.py): dW2 / dW1 with the bias gradient (rowsum) fused, K = the batch of 2 x 256 views
    for pout, pin, n in ((128, 128, 512), (128, 2048, 512), (2048, 2048, 1024)):
        d = _desc(L, pout, pin, n, rowsum=True)
        default = _name(L, [d], 2)
        bvc.use_deterministic_algorithms(True)
        det = _name(L, [d], 2)
        assert det.startswith("bvc::gemm_det_kernel<") and det.endswith("true, true>"), det
        bvc.use_deterministic_algorithms(False)
        assert _name(L, [d], 2) == default and default.startswith("bvc::gemm_kernel<")


def test_explicit_persistent_tile_configs_map_onto_the_deterministic_kernel(L, bvc):
    # tile configs 6 / 7 / 9 name the persistent kernels, which take no split / accumulating / bias-gradient outputs: in deterministic
    # mode such problems run on the 128 x 128 / 128 x 64 deterministic kernel
    bvc.use_deterministic_algorithms(True)
    for tile, want in ((6, "bvc::gemm_det_kernel<128, 128, true, true>"), (9, "bvc::gemm_det_kernel<128, 128, true, true>"),
                       (7, "bvc::gemm_det_kernel<128, 64, true, true>")):
        assert _name(L, [_desc(L, 768, 3072, 2560, split=4)], 2, tile) == want, tile
        assert _name(L, [_desc(L, 768, 3072, 2560, rowsum=True)], 2, tile) == want, tile
