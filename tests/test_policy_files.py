"""The policy checkpoint loader's validation (csrc/policy.cpp,
mpenv_policy_check): a written checkpoint passes, and each way a directory can
be wrong is refused with the file and the reason named.  No GPU."""
import os
import struct

import numpy as np
import pytest

import policy_testlib as P

ERR_INVALID, ERR_IO = -1, -2
SELF_EMBED = "params_backbone_prefix_self_embed_kernel"
TRUNK_1 = "params_backbone_actor_encoder_net_MaxPoolNet_0_MLP_0_Dense_1_kernel"
HEAD_1 = "params_actor_DenseLayerDiscreteActor_1_impl_kernel"


@pytest.fixture()
def ckpt(tmp_path):
    d = tmp_path / "ckpt"
    return d, P.write_checkpoint(d, 11)


def test_written_checkpoint_passes_and_has_every_file(ckpt):
    d, tensors = ckpt
    assert P.policy_check(d) == (0, "")
    # 14 normalisation files, 6 x 3 embed, 3 x 3 trunk, 2 x 2 heads
    assert len(tensors) == 14 + 18 + 9 + 4 == len(os.listdir(d))
    # the dense parameters are the 772,864 floats of the architecture
    assert sum(v.size for k, v in tensors.items() if k.endswith("_kernel")) == 772864


def test_file_format_is_ndim_shape_data(ckpt):
    d, tensors = ckpt
    raw = open(d / SELF_EMBED, "rb").read()
    assert struct.unpack("<3i", raw[:12]) == (2, 100, 64)
    assert np.array_equal(np.frombuffer(raw[12:], np.float32).reshape(100, 64), tensors[SELF_EMBED])


@pytest.mark.parametrize("name", ["obs_preprocess_state_opponents_last_known_inv_sigma", TRUNK_1,
                                  "params_backbone_prefix_LayerNorm_4_impl_bias",
                                  "params_actor_DenseLayerDiscreteActor_0_impl_bias"])
def test_missing_file(ckpt, name):
    d, _ = ckpt
    os.remove(d / name)
    rc, msg = P.policy_check(d)
    assert rc == ERR_IO and name in msg and "cannot open" in msg, msg


def test_missing_directory(tmp_path):
    rc, msg = P.policy_check(tmp_path / "nowhere")
    assert rc == ERR_IO and "cannot open" in msg, msg


@pytest.mark.parametrize("keep", [0, 2, 8, 12 + 4 * 511])
def test_truncated_file(ckpt, keep):
    d, _ = ckpt
    raw = open(d / TRUNK_1, "rb").read()
    open(d / TRUNK_1, "wb").write(raw[:keep])
    rc, msg = P.policy_check(d)
    assert rc == ERR_IO and TRUNK_1 in msg and "truncated" in msg, msg


def test_wrong_rank(ckpt):
    d, tensors = ckpt
    P.write_tensor(d / SELF_EMBED, tensors[SELF_EMBED].reshape(-1))
    rc, msg = P.policy_check(d)
    assert rc == ERR_INVALID and SELF_EMBED in msg and "rank 1" in msg, msg
    P.write_tensor(d / SELF_EMBED, tensors[SELF_EMBED])
    bias = "params_backbone_prefix_LayerNorm_2_impl_bias"
    P.write_tensor(d / bias, tensors[bias].reshape(8, 8))
    rc, msg = P.policy_check(d)
    assert rc == ERR_INVALID and bias in msg and "rank 2" in msg, msg


@pytest.mark.parametrize("name,shape,got", [
    (SELF_EMBED, (99, 64), "99 x 64"),      # an embed: SelfObservation without the position embedding etc.
    (SELF_EMBED, (64, 100), "64 x 100"),    # [out][in] instead of [in][out]
    (TRUNK_1, (384, 512), "384 x 512"),     # a trunk layer
    (HEAD_1, (512, 17), "512 x 17"),        # a head: the discrete head's width on the aim head
    ("obs_preprocess_state_self_mu", (44,), "44"),
])
def test_wrong_shape(ckpt, name, shape, got):
    d, _ = ckpt
    P.write_tensor(d / name, np.zeros(shape, np.float32))
    rc, msg = P.policy_check(d)
    assert rc == ERR_INVALID and name in msg and f"wrong shape {got}" in msg, msg
