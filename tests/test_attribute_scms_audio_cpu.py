"""The AudioMNIST attribute SCM without a GPU: the statement of the log-probabilities, ``sample_differing`` on CPU
tensors (the statement of the kernels' "differ" mode), the host plan of csrc/cat.hip, ``CatState.matches``, and ``train``
on CPU tensors."""
import numpy as np
import pytest
import torch

import cat_cases as cc


def test_statement_log_prob_is_categorical_of_the_modules_logits():
    sizes = cc.SIZES["wide"]
    g = cc.twin(cc.new_graph(sizes, 1), sizes, torch.float64)
    country, native, accent = (t.double() for t in cc.contexts(sizes, 40, "onehot"))
    lp = g.log_prob({"country_of_origin": country, "native_speaker": native, "accent": accent})
    zn, za = cc.statement_logits(g, country, native, torch.float64)
    for key, z, y in (("native_speaker", zn, native), ("accent", za, accent)):
        want = torch.distributions.Categorical(logits=z).log_prob(y.argmax(1))
        assert lp[key].shape == (40,) and lp[key].dtype == torch.float64
        assert torch.allclose(lp[key], want, rtol=0, atol=1e-12)
        assert torch.allclose(lp[key], torch.log_softmax(z, 1).gather(1, y.argmax(1, keepdim=True))[:, 0], rtol=0, atol=1e-12)


def test_sample_differing_never_returns_the_forbidden_class():
    sizes = cc.SIZES["small"]
    g = cc.new_graph(sizes, 2)
    torch.manual_seed(5)
    n = 500
    country = torch.randint(0, sizes[0], (n,))
    for key, C in (("native_speaker", sizes[1]), ("accent", sizes[2])):
        forb = torch.randint(0, C, (n,))
        out, status = g.sample_differing({"country_of_origin": country}, key, forb)
        assert status.shape == (n,) and status.dtype == torch.int32 and int(status.sum()) == 0
        assert out[key].shape == (n,) and out[key].dtype == torch.int64
        assert not (out[key] == forb).any() and int(out[key].max()) < C
        assert out["country_of_origin"] is country and set(out) == set(g.modules)


def test_sample_differing_reports_a_one_class_node():
    g = cc.new_graph(cc.CORNER, 3)
    out, status = g.sample_differing({"country_of_origin": torch.zeros(7, dtype=torch.int64)}, "accent",
                                     torch.zeros(7, dtype=torch.int64))
    assert torch.equal(status, torch.ones(7, dtype=torch.int32)) and torch.equal(out["accent"], torch.zeros(7, dtype=torch.int64))


def test_sample_differing_frequencies_are_the_renormalised_softmax():
    sizes = cc.SIZES["small"]
    g = cc.new_graph(sizes, 4)
    n, Ca = 20_000, sizes[2]
    country = torch.full((n,), 2, dtype=torch.int64)
    native = torch.ones(n, dtype=torch.int64)
    _, za = cc.statement_logits(g, torch.eye(sizes[0])[country[:1]], torch.eye(sizes[1])[native[:1]], torch.float32)
    p = torch.softmax(za[0].double(), 0)
    f = int(p.argmax())                                     # forbid the likeliest class: the loop has work to do
    torch.manual_seed(11)
    out, status = g.sample_differing({"country_of_origin": country, "native_speaker": native}, "accent",
                                     torch.full((n,), f, dtype=torch.int64))
    assert int(status.sum()) == 0
    q = p.clone()
    q[f] = 0
    q /= q.sum()
    freq = torch.bincount(out["accent"], minlength=Ca).double() / n
    se = (q * (1 - q) / n).sqrt()
    print("frequencies", freq.tolist(), "renormalised softmax", q.tolist())
    assert freq[f] == 0 and ((freq - q).abs() <= 4 * se + 1e-12).all()


def test_plan_refusals_workspace_and_row_cover():
    from ali_hip import ops
    for bad in ((0, 2, 6), (5, 65, 6), (5, 2, 0), (65, 2, 6)):
        with pytest.raises(RuntimeError, match="class counts"):
            ops.cat_plan(100, *bad)
    with pytest.raises(RuntimeError, match="N = 0"):
        ops.cat_plan(0, 5, 2, 6)
    with pytest.raises(RuntimeError, match="entry"):
        ops.cat_plan(10, 5, 2, 6, entry=7)
    assert ops.cat_plan(100, 5, 2, 6, ops.CAT_ENTRY_MAP).ws_bytes == 0
    last = 0
    for N in (1, 31, 32, 33, 257, 4096, 8192, 8193, 10_000, 100_000):
        for entry in (ops.CAT_ENTRY_NLL, ops.CAT_ENTRY_GRAD, ops.CAT_ENTRY_MAP):
            pl = ops.cat_plan(N, 13, 2, 17, entry)
            seen = np.zeros(N, dtype=np.int64)
            for b in range(pl.grid):
                tiles = [b + j * pl.grid for j in range(pl.tiles_per_block) if b + j * pl.grid < pl.tiles]
                assert tiles, "no idle block"
                for t in tiles:
                    seen[t * pl.tile_rows:min(N, (t + 1) * pl.tile_rows)] += 1
            assert (seen == 1).all(), (N, entry)
            assert pl.lds_bytes <= 160 * 1024 and pl.threads <= 1024 and pl.threads2 <= 1024
        ws = ops.cat_plan(N, 13, 2, 17, ops.CAT_ENTRY_GRAD).ws_bytes
        assert ws > last and ws >= ops.cat_plan(N, 13, 2, 17, ops.CAT_ENTRY_NLL).ws_bytes
        last = ws
    theta, towers = ops.cat_sizes(5, 2, 6)
    assert theta == sum(p.numel() for p in cc.trained_params(cc.new_graph(cc.SIZES["small"])))
    assert towers == sum(m.weight.numel() + m.bias.numel() for m in cc.linears(cc.new_graph(cc.SIZES["small"]))[4:12])


def test_cat_state_matches_follows_the_graph():
    """``matches`` without a device: the checks are on structure, identity and storage"""
    from ali_hip import cat
    sizes = cc.SIZES["small"]
    g = cc.new_graph(sizes, 5)
    found = cat._layers(g)
    assert found is not None and found[2] == sizes and len(found[0]) == 6 and len(found[1]) == 8
    st = cat.CatState.__new__(cat.CatState)                # bind's bookkeeping on CPU buffers
    st.trained, st.frozen, st.sizes = found
    st.theta, st.params = cat._flatten(st.trained, sum(p.numel() for p in cc.trained_params(g)), torch.device("cpu"))
    st.towers, st.tower_params = cat._flatten(st.frozen, sum(m.weight.numel() + m.bias.numel() for m in st.frozen),
                                              torch.device("cpu"))
    st.mods = tuple(g.get_module(k) for k in cat.NODES + cat.ROOTS)
    assert st.matches(g)
    assert all(a is b for a, b in zip(st.params, cc.trained_params(g)))          # parameters() still reaches them
    g.add_edge("age", "accent")
    assert not st.matches(g)
    g.remove_edge("age", "accent")
    assert st.matches(g)
    ns = g.get_module("native_speaker").model
    old = ns[2]
    ns[2] = torch.nn.Linear(128, 128)
    assert not st.matches(g)
    ns[2] = old
    assert st.matches(g)
    old_w = ns[0].weight
    ns[0].weight = torch.nn.Parameter(old_w.detach().clone())
    assert not st.matches(g)
    ns[0].weight = old_w
    assert st.matches(g)
    old_data = old_w.data
    old_w.data = old_data.clone()                            # the same parameter, moved out of the flat buffer
    assert not st.matches(g)
    old_w.data = old_data
    assert st.matches(g)
    ns[1] = torch.nn.Tanh()
    assert not st.matches(g)


def test_train_on_cpu_tensors_lowers_the_loss():
    import attribute_scms.audio_mnist as aa
    torch.manual_seed(0)
    np.random.seed(0)
    g = aa.train(cc.onehot_ds(cc.SIZES["small"], 300, 1), steps=2, device="cpu")
    assert len(g.train_losses) == 2 and g.train_losses[1] < g.train_losses[0]
    assert g._cat is None
