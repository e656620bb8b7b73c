"""Wide split mode (conv_algo=5), the part that needs no GPU: the construction-time check of Config."""
import pytest
import torch


def test_config_rejects_wide_split_with_bf16_tensors():
    from coma_unet_amd.layers import Config
    with pytest.raises(ValueError, match="conv_algo=5"):
        Config(compute_dtype=torch.bfloat16, conv_algo=5)
    assert Config(compute_dtype=torch.float32, conv_algo=5).conv_algo == 5
    with pytest.raises(ValueError, match="conv_algo=4"):
        Config(compute_dtype=torch.bfloat16, conv_algo=4)


def test_build_model_takes_wide_split():
    import coma_unet_amd as cu
    with pytest.raises(ValueError, match="conv_algo=5"):
        cu.build_model(volume_shape=(32, 32, 32), compute_dtype=torch.bfloat16, conv_algo=5)
