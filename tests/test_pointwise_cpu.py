"""conv_algo=7 (pointwise fp32 MFMA) at the host level: it keeps fp32 tensors, so a bf16 compute dtype is refused like for 4, 5
and 6."""
import pytest
import torch


def test_config_refuses_bf16_tensors():
    from coma_unet_amd.layers import Config
    with pytest.raises(ValueError, match="conv_algo=7"):
        Config(compute_dtype=torch.bfloat16, conv_algo=7)


def test_build_model_refuses_bf16_tensors():
    import coma_unet_amd as cu
    with pytest.raises(ValueError, match="conv_algo=7"):
        cu.build_model(volume_shape=(32, 32, 32), compute_dtype=torch.bfloat16, conv_algo=7)


def test_config_keeps_the_mode():
    from coma_unet_amd.layers import Config
    assert Config(compute_dtype=torch.float32, conv_algo=7).conv_algo == 7
