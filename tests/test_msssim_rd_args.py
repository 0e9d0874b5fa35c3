"""CPU checks of the differentiable MS-SSIM surface: the two backward symbols are exported and validate their arguments without
touching a device, and `args.rd_metric` of the R + lambda*D calibration mode is checked before any work is done."""
import types

import pytest
import torch


def test_backward_symbols_are_exported_and_validate_arguments():
    import ctypes as C
    from hipops import _lib as L
    h = L.lib()
    assert "rdo_ssim_level_bwd" in L.EXPORTS and "rdo_avg_pool2_bwd" in L.EXPORTS
    win = (C.c_float * 11)(*([1.0 / 11] * 11))
    assert h.rdo_ssim_level_bwd(None, None, 1, 64, 64, win, 1e-4, 9e-4, None, None, None, None) != 0
    assert h.rdo_avg_pool2_bwd(None, 1, 64, 64, None, None) != 0


def test_avg_pool2_bwd_checks_the_gradient_shape():
    from hipops import ops
    with pytest.raises(ValueError):
        ops.avg_pool2_bwd(torch.zeros(3, 10, 10), 21, 20)          # a 21 x 20 input pools to 11 x 10


@pytest.mark.parametrize("metric,side,ok", [("mse", 64, True), ("ms-ssim", 176, True), ("ms-ssim", 160, False), ("ms-ssim", 64, False),
                                            ("nope", 176, False), ("ssim", 64, False)])
def test_rd_metric_argument(metric, side, ok):
    from quantization.recon import _rd_metric
    args = types.SimpleNamespace(loss_mode="rd", rd_metric=metric)
    cali = torch.zeros(2, 3, side, side + 8)
    if ok:
        assert _rd_metric(args, cali) == metric
    else:
        with pytest.raises(ValueError, match="ms-ssim"):
            _rd_metric(args, cali)


def test_rd_metric_defaults_to_mse_and_is_refused_before_any_work():
    from quantization import layer_reconstruction
    from quantization.recon import _rd_metric
    assert _rd_metric(types.SimpleNamespace(loss_mode="rd"), torch.zeros(1, 3, 64, 64)) == "mse"
    assert _rd_metric(None, torch.zeros(1, 3, 64, 64)) == "mse"
    # refused before the model, the unit or a device is looked at
    for metric, side in (("nope", 176), ("ms-ssim", 64)):
        with pytest.raises(ValueError, match="ms-ssim"):
            layer_reconstruction(None, None, "0", torch.zeros(2, 3, side, side), batch_size=2, iters=1,
                                 args=types.SimpleNamespace(loss_mode="rd", rd_metric=metric, task_loss=2.0))


def test_ssim_level_bwd_checks_shapes():
    from hipops import ops
    x = torch.zeros(3, 20, 20)
    with pytest.raises(ValueError):
        ops.ssim_level_bwd(x, torch.zeros(3, 20, 21), [1.0 / 11] * 11, 1e-4, 9e-4, torch.zeros(3), torch.zeros(3))
    with pytest.raises(ValueError):
        ops.ssim_level_bwd(x, x, [1.0 / 11] * 11, 1e-4, 9e-4, torch.zeros(2), torch.zeros(3))
