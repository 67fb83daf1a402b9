"""``ChainPlan`` refuses, at construction, every layer setting its stages cannot represent -- they keep ``stride[0]``,
``padding[0]``, ``output_padding[0]`` and nothing else of a convolution -- and names the layer's index in the Sequential
and the setting.  None of the stacks the package itself hands to ``get_plan`` / ``run_chain`` is refused.

No GPU: everything is built on the meta device."""
import importlib

import pytest
import torch
import torch.nn as nn

C, CT, BN = nn.Conv2d, nn.ConvTranspose2d, nn.BatchNorm2d

# id -> (layers in front of the offender, the offender, what the message must name)
REFUSED = {
    "conv_stride": ([], lambda: C(4, 8, 3, stride=(2, 1)), r"stride=\(2, 1\)"),
    "conv_padding": ([], lambda: C(4, 8, 3, padding=(1, 0)), r"padding=\(1, 0\)"),
    "conv_padding_same": ([], lambda: C(4, 8, 3, padding="same"), r"padding='same'"),
    "conv_padding_valid": ([], lambda: C(4, 8, 3, padding="valid"), r"padding='valid'"),
    "conv_dilation": ([], lambda: C(4, 8, 3, dilation=2), r"dilation=\(2, 2\)"),
    "conv_groups": ([], lambda: C(4, 8, 3, groups=2), r"groups=2"),
    "conv_padding_mode": ([], lambda: C(4, 8, 3, padding=1, padding_mode="reflect"), r"padding_mode='reflect'"),
    "convT_stride": ([], lambda: CT(4, 8, 3, stride=(1, 2)), r"stride=\(1, 2\)"),
    "convT_padding": ([], lambda: CT(4, 8, 3, padding=(0, 1)), r"padding=\(0, 1\)"),
    "convT_output_padding": ([], lambda: CT(4, 8, 3, stride=2, output_padding=(1, 0)), r"output_padding=\(1, 0\)"),
    "convT_dilation": ([], lambda: CT(4, 8, 3, dilation=2), r"dilation=\(2, 2\)"),
    "convT_groups": ([], lambda: CT(4, 8, 3, groups=2), r"groups=2"),
    "bn_momentum_none": ([lambda: C(4, 8, 3), lambda: nn.LeakyReLU(0.2)], lambda: BN(8, momentum=None), r"momentum=None"),
    "bn_not_affine": ([lambda: C(4, 8, 3), lambda: nn.LeakyReLU(0.2)], lambda: BN(8, affine=False), r"affine=False"),
    "unflatten_dim": ([lambda: nn.Linear(4, 8)], lambda: nn.Unflatten(-1, (8, 1, 1)), r"dim=-1"),
    "dropout_p_one": ([lambda: C(4, 8, 3)], lambda: nn.Dropout2d(1.0), r"p=1\.0"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_unsupported_setting_is_refused_by_name(case):
    from ali_hip.chain import ChainPlan
    front, bad, names = REFUSED[case]
    with torch.device("meta"):
        mods = [f() for f in front] + [bad()] + [nn.Conv2d(8, 4, 1)]
        seq = nn.Sequential(*mods)
    index = len(front)
    with pytest.raises(NotImplementedError, match=rf"layer {index} \({type(mods[index]).__name__}\): {names}"):
        ChainPlan(seq)


def test_taped_dropout_is_checked_like_dropout2d():
    import ali_oracle
    from ali_hip.chain import ChainPlan
    with torch.device("meta"):
        seq = nn.Sequential(ali_oracle.TapedDropout2d(-0.1), nn.Conv2d(4, 4, 1))
    with pytest.raises(NotImplementedError, match=r"layer 0 \(TapedDropout2d\): p=-0\.1"):
        ChainPlan(seq)


def test_supported_settings_still_plan():
    from ali_hip.chain import ChainPlan
    with torch.device("meta"):
        ChainPlan(nn.Sequential(nn.Dropout2d(0.0), C(4, 8, (3, 2), stride=(2, 2), padding=(1, 1), bias=False),
                                BN(8, track_running_stats=False), CT(8, 4, (2, 3), stride=2, padding=1, output_padding=1),
                                nn.Flatten(), nn.Linear(16, 4, bias=False)))
        ChainPlan(nn.Sequential(nn.Linear(4, 8), nn.Unflatten(1, (8, 1, 1)), nn.ReLU(), BN(8, momentum=0.3), C(8, 1, 1)))


def _shipped():
    """name -> nn.Sequential, every stack a ``get_plan`` / ``run_chain`` call site of the package passes (image_scms,
    deepscm_vae, gans, classifiers, ali_hip/cfmetrics.py, vae.py, gan.py, explain.py: decoders and classifiers)"""
    from ali_hip.vae import head_chains
    out = {}
    for fam in ("mnist", "audio_mnist", "whalecalls", "esrf_acoustic"):
        pm = importlib.import_module("image_scms." + fam)
        E, G, D = pm.Encoder(), pm.Generator(), pm.Discriminator()
        out.update({f"image_scms.{fam}.E": E.layers, f"image_scms.{fam}.G": G.layers, f"image_scms.{fam}.dx": D.dx,
                    f"image_scms.{fam}.dz": D.dz, f"image_scms.{fam}.dxz": D.dxz})
    for fam in ("mnist", "audio_mnist", "whalecalls"):
        pm = importlib.import_module("deepscm_vae." + fam)
        enc, dec = pm.VAEEncoder(), pm.VAEDecoder()
        hm, hv = head_chains(enc)
        out.update({f"deepscm_vae.{fam}.encoder": enc.layers, f"deepscm_vae.{fam}.mean": hm,
                    f"deepscm_vae.{fam}.log_var": hv, f"deepscm_vae.{fam}.decoder": dec.layers})
    import gans.audio_mnist as gm
    out.update({"gans.audio_mnist.G": gm.Generator().layers, "gans.audio_mnist.D": gm.Discriminator().layers})
    import classifiers.audio_mnist
    import classifiers.mnist
    import classifiers.whalecalls
    out.update({"classifiers.mnist": classifiers.mnist.MNISTClassifier(),
                "classifiers.audio_mnist": classifiers.audio_mnist.AudioMNISTClassifier(),
                "classifiers.whalecalls": classifiers.whalecalls.NARWClassifier()})
    import train_morphomnist_ae as ae
    out.update({"cfmetrics.E": ae.Encoder().chain_view(), "cfmetrics.G": ae.Decoder().chain_view()})
    return out


def test_no_shipped_stack_is_refused():
    from ali_hip.chain import ChainPlan
    with torch.device("meta"):
        seqs = _shipped()
    assert len(seqs) == 39
    for name, seq in seqs.items():
        assert isinstance(seq, nn.Sequential), name
        plan = ChainPlan(seq)
        assert plan.stages, name
