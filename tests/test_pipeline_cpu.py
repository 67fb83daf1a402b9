"""``ali_hip.pipeline`` without a device: what ``Decoder`` reads off the two kinds of generator stack, and
``require_eval``.  The refusals of foreign decoders and classifiers are asserted where the executors are built
(test_explain_cpu.py, test_attrib_cpu.py, test_contrastive_cpu.py); the passes and the layout cache need a device
(test_gpu_explainer_bits.py and the executors' own GPU tests)."""
import pytest
import torch


def test_decoder_of_the_mnist_generator():
    import image_scms.mnist as pm
    from ali_hip.pipeline import Decoder
    G = pm.Generator()
    dec = Decoder(G)
    attrs = {"thickness": None, "digit": None, "slant": None, "intensity": None}       # (any order: the row's is fixed)
    cat, cont = dec.keys(attrs)
    assert (cat, cont) == (["digit"], ["intensity", "slant", "thickness"])
    assert dec.keys({"digit": None, "thickness": None}) == (["digit"], ["thickness"])
    with pytest.raises(ValueError, match="the decoder takes the attributes"):
        dec.keys({"thickness": None})                                                  # no digit
    tables = dec.tables(cat)
    assert len(tables) == 1 and tables[0].data_ptr() == G.digit_embedding.weight.data_ptr()
    assert tuple(tables[0].shape) == (10, 256) and not tables[0].requires_grad
    assert dec.latent() == 512 and dec.image_hw() == (28, 28) and dec.layers is G.layers
    assert dec.row_width(cat, cont) == (512 + 256 + 3, 800)                            # 771 -> the next multiple of 32
    assert dec.row_width(cat, []) == (768, 768)                                        # already one: no padding
    assert dec.row_width(cat, cont)[0] == G.layers[0].in_channels


def test_decoder_of_a_spectrogram_generator():
    import image_scms.audio_mnist as am
    from ali_hip.pipeline import Decoder
    G = am.Generator(8)
    dec = Decoder(G)
    cat, cont = dec.keys(dict.fromkeys(am.ATTRIBUTE_DIMS))
    assert cat == sorted(am.ATTRIBUTE_DIMS) and cont == []
    with pytest.raises(ValueError, match="the decoder takes the attributes"):
        dec.keys({"digit": None})
    tables = dec.tables(cat)
    assert [t.data_ptr() for t in tables] == [G.embedding_dict[k].weight.data_ptr() for k in cat]
    assert [tuple(t.shape) for t in tables] == [(am.ATTRIBUTE_DIMS[k], 256) for k in cat]
    assert dec.latent() == 512 and dec.image_hw() == (128, 128) and dec.layers is G.layers
    assert dec.row_width(cat, cont) == (512 + 6 * 256, 2048)
    first = next(m for m in G.layers.modules() if hasattr(m, "in_features") or hasattr(m, "in_channels"))
    assert dec.row_width(cat, cont)[0] == (first.in_features if hasattr(first, "in_features") else first.in_channels)
    assert dec.row_width(cat[:1], ["c"]) == (769, 800)


def test_require_eval_names_the_caller_and_the_module():
    from ali_hip.pipeline import require_eval
    a, b = torch.nn.Linear(1, 1).eval(), torch.nn.Linear(1, 1).eval()
    require_eval("Someone", decoder=a, classifier=b)
    require_eval("Someone")
    b.train()
    with pytest.raises(ValueError, match=r"Someone: the classifier is in training mode.*eval mode only.*\.eval\(\)"):
        require_eval("Someone", decoder=a, classifier=b)
    a.train()
    with pytest.raises(ValueError, match="Someone: the decoder is in training mode"):  # the first one named
        require_eval("Someone", decoder=a, classifier=b)
