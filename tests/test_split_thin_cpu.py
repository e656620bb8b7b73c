"""conv_algo=6 (thin split) at the host level: it keeps fp32 tensors, so a bf16 compute dtype is refused like for 4 and 5."""
import pytest
import torch


def test_config_refuses_bf16_tensors():
    from coma_unet_amd.layers import Config
    with pytest.raises(ValueError, match="conv_algo=6"):
        Config(compute_dtype=torch.bfloat16, conv_algo=6)


def test_build_model_refuses_bf16_tensors():
    import coma_unet_amd as cu
    with pytest.raises(ValueError, match="conv_algo=6"):
        cu.build_model(volume_shape=(32, 32, 32), compute_dtype=torch.bfloat16, conv_algo=6)


def test_config_keeps_the_mode():
    from coma_unet_amd.layers import Config
    assert Config(compute_dtype=torch.float32, conv_algo=6).conv_algo == 6
