"""The cf_eval family without a GPU: ``ManifoldBank`` on CPU tensors against the loop of audiomnist_cf_eval.py:93-131
written out here, the moment identity the kernels of csrc/cfeval.hip evaluate against that pairwise statement in fp64,
and ``CounterfactualEval`` on the stock CPU modules against the loop bodies of audiomnist_cf_eval.py,
audiomnist_cf_classifier_metric.py and mnist_bigan_score.py.  ``bank_case`` and ``moment_errors`` also serve the GPU
tests."""
import numpy as np
import pytest
import torch


def bank_case(N, D, O, C, M, seed=0, dtype=torch.float32):
    """(rows [N, D], owner [N], cls [N], cf [M, D], cf_owner [M], cf_cls [M]): images in [-1, 1], every label in range"""
    g = torch.Generator().manual_seed(seed * 7919 + N * 131 + D * 17 + O * 5 + C + M)
    rows = (torch.rand(N, D, generator=g) * 2 - 1).to(dtype)
    owner, cls = torch.randint(0, O, (N,), generator=g), torch.randint(0, C, (N,), generator=g)
    cf = (torch.rand(M, D, generator=g) * 2 - 1).to(dtype)
    return rows, owner, cls, cf, torch.randint(0, O, (M,), generator=g), torch.randint(0, C, (M,), generator=g)


def script_loop(rows, r_owner, r_cls, cf, owner, cls, batch=7):
    """audiomnist_cf_eval.py:93-131, one (subject, d) at a time: masks, ``unsqueeze(1)``, the "other" sum accumulated
    over streamed batches of ``batch`` recordings that exclude the subject, ``/ denom``"""
    M = cf.shape[0]
    same, other = cf.new_empty(M), cf.new_empty(M)
    for o, d in sorted(set(zip(owner.tolist(), cls.tolist()))):
        at = (owner == o) & (cls == d)
        img = cf[at]
        same_mask = (r_owner == o) & (r_cls == d)
        same_x = rows[same_mask]
        same_err = (img.unsqueeze(1) - same_x).square().sum(dim=(1, 2)) / len(same_x)
        other_err = torch.zeros((len(img),), dtype=cf.dtype)
        denom = 0
        keep = r_owner != o                                       # data.stream(excluded_subjects=[subject])
        s_rows, s_cls = rows[keep], r_cls[keep]
        for lo in range(0, len(s_rows), batch):
            other_mask = s_cls[lo:lo + batch] == d
            other_x = s_rows[lo:lo + batch][other_mask]
            other_err += (img.unsqueeze(1) - other_x).square().sum(dim=(1, 2))
            denom += len(other_x)
        other_err /= denom
        same[at], other[at] = same_err, other_err
    return {"same": same, "other": other, "ratio": same / other}


def moment_errors(rows, r_owner, r_cls, cf, owner, cls, O, C):
    """What csrc/cfeval.hip evaluates, in fp64 torch ops: the cells' column sums S and sums of squares Q, the class
    totals folded over the owners in ascending order from 0, then per row sum_k (n a^2 - 2 a S + Q) / n and the same on
    (TS - S, TQ - Q, tcnt - n).  Every label in range."""
    D = rows.shape[1]
    r64, a = rows.double(), cf.double()
    cell = r_owner * C + r_cls
    S = torch.zeros(O * C, D, dtype=torch.float64).index_add_(0, cell, r64)
    Q = torch.zeros(O * C, D, dtype=torch.float64).index_add_(0, cell, r64 * r64)
    cnt = torch.bincount(cell, minlength=O * C)
    TS, TQ = torch.zeros(C, D, dtype=torch.float64), torch.zeros(C, D, dtype=torch.float64)
    for o in range(O):
        TS += S.reshape(O, C, D)[o]
        TQ += Q.reshape(O, C, D)[o]
    tcnt = cnt.reshape(O, C).sum(0)
    at = owner * C + cls
    n, m = cnt[at].double().reshape(-1, 1), (tcnt[cls] - cnt[at]).double().reshape(-1, 1)
    a2 = a * a
    same = ((n * a2 - 2.0 * a * S[at]) + Q[at]).sum(1) / n[:, 0]
    other = ((m * a2 - 2.0 * a * (TS[cls] - S[at])) + (TQ[cls] - Q[at])).sum(1) / m[:, 0]
    return {"same": same, "other": other, "ratio": same / other}


def full_case(N=60, D=63, O=3, C=2, M=9, seed=1):
    """a case in which every cell and every rest of a class holds rows"""
    for s in range(seed, seed + 50):
        rows, ro, rc, cf, o, c = bank_case(N, D, O, C, M, s, torch.float64)
        cnt = torch.bincount(ro * C + rc, minlength=O * C).reshape(O, C)
        if (cnt > 0).all() and (O == 1 or ((cnt.sum(0, keepdim=True) - cnt) > 0).all()):
            return rows, ro, rc, cf, o, c
    raise AssertionError("no full case")


# ------------------------------------------------------------------------------------------------------ ManifoldBank
def test_bank_errors_in_fp64_equal_the_scripts_loop():
    from ali_hip.cfeval import ManifoldBank
    rows, ro, rc, cf, o, c = full_case()
    got = ManifoldBank(rows.reshape(-1, 7, 9), ro, rc, 3, 2).errors(cf.reshape(-1, 7, 9), o, c)
    want = script_loop(rows, ro, rc, cf, o, c)
    assert set(got) == {"same", "other", "ratio"} and got["same"].dtype == torch.float64
    for k in want:
        assert torch.isfinite(want[k]).all()
        np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("D,N", [(1, 12), (63, 40), (784, 60)])
def test_moment_identity_in_fp64_against_the_pairwise_statement(D, N):
    """fp32 inputs, as the kernels get them.  Per column the identity's terms are of the size n a^2 <= n and carry a
    few fp64 roundings (1.1e-16 each) while the column's result is sum_j (a - b_j)^2: about n / 3 for independent rows
    (relative error ~1e-15) and n * 1e-6 for the rows placed 1e-3 from a bank row of a one-row cell (~1e-9).  Bounds:
    1e-12 and 1e-7; rounded to fp32 the two agree to an ulp either way."""
    from ali_hip.cfeval import ManifoldBank
    rows, ro, rc, cf, o, c = (t.float() if t.is_floating_point() else t for t in full_case(N, D, 3, 2, 9, seed=D))
    bank = ManifoldBank(rows.double(), ro, rc, 3, 2)
    want = bank.errors(cf.double(), o, c)
    got = moment_errors(rows, ro, rc, cf, o, c, 3, 2)
    for k in want:
        np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), rtol=1e-12, atol=0)
        ulp = (got[k].float().double() - want[k].float().double()).abs() / (want[k].abs() * 2.0 ** -23)
        assert ulp.max() <= 1.0, (k, ulp.max())
    # rows 1e-3 from the only row of their cell
    rows1 = torch.cat([rows, (torch.rand(1, D, generator=torch.Generator().manual_seed(5)) * 2 - 1)])
    ro1, rc1 = torch.cat([ro, torch.tensor([3])]), torch.cat([rc, torch.tensor([1])])
    sign = torch.where(torch.arange(D) % 2 == 0, 1.0, -1.0)
    near = torch.stack([rows1[-1] + 1e-3 * sign, rows1[-1] - 1e-3 * sign, rows1[-1]])
    no, nc = torch.tensor([3, 3, 3]), torch.tensor([1, 1, 1])
    want = ManifoldBank(rows1.double(), ro1, rc1, 4, 2).errors(near.double(), no, nc)
    got = moment_errors(rows1, ro1, rc1, near, no, nc, 4, 2)
    assert want["same"][2] == 0.0 and got["same"][2] == 0.0 and got["ratio"][2] == 0.0
    np.testing.assert_allclose(got["same"][:2].numpy(), want["same"][:2].numpy(), rtol=1e-7, atol=0)
    np.testing.assert_allclose(got["other"].numpy(), want["other"].numpy(), rtol=1e-12, atol=0)


def corner_case(dtype=torch.float64):
    """O = 3, C = 3: cell (0, 0) empty while class 0 has rows; class 1 held by owner 1 alone; class 2 ordinary.  The
    rows ask for: an empty cell, an empty rest of the class, an unseen owner (3, -1), a class out of range (3, -2), and
    two ordinary cells.  Returns (rows, owner, cls, cf, cf_owner, cf_cls, expected NaN mask [M, 3])."""
    g = torch.Generator().manual_seed(3)
    ro = torch.tensor([1, 2, 1, 1, 0, 1, 2, 2, 0])
    rc = torch.tensor([0, 0, 1, 1, 2, 2, 2, 0, 2])
    rows = (torch.rand(len(ro), 20, generator=g) * 2 - 1).to(dtype)
    o = torch.tensor([0, 1, 3, -1, 1, 0, 2, 1])
    c = torch.tensor([0, 1, 2, 0, 3, -2, 2, 0])
    cf = (torch.rand(len(o), 20, generator=g) * 2 - 1).to(dtype)
    T, F = True, False
    nan = torch.tensor([[T, F, T], [F, T, T], [T, F, T], [T, F, T], [T, T, T], [T, T, T], [F, F, F], [F, F, F]])
    return rows, ro, rc, cf, o, c, nan


def test_the_four_nan_corners():
    from ali_hip.cfeval import ManifoldBank
    rows, ro, rc, cf, o, c, nan = corner_case()
    e = ManifoldBank(rows, ro, rc, 3, 3).errors(cf, o, c)
    got = torch.stack([e["same"], e["other"], e["ratio"]], dim=1)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.isfinite(got[~nan]).all() and (got[~nan] > 0).all()
    # an unseen owner is measured against the whole class
    whole = (cf[2].unsqueeze(0) - rows[rc == 2]).square().sum() / int((rc == 2).sum())
    np.testing.assert_allclose(e["other"][2].item(), whole.item(), rtol=1e-12)


def test_left_out_bank_rows_and_one_hot_labels():
    from ali_hip.cfeval import ManifoldBank
    rows, ro, rc, cf, o, c = full_case()
    want = ManifoldBank(rows, ro, rc, 3, 2).errors(cf, o, c)
    g = torch.Generator().manual_seed(9)
    junk = torch.rand(4, rows.shape[1], generator=g, dtype=torch.float64)
    at = torch.tensor([0, 17, 17, 40])                                        # where the junk rows go
    keep = torch.ones(len(rows) + 4, dtype=torch.bool)
    slots = at + torch.arange(4)
    keep[slots] = False
    rows2 = torch.empty(len(rows) + 4, rows.shape[1], dtype=torch.float64)
    ro2, rc2 = torch.empty(len(rows) + 4, dtype=torch.long), torch.empty(len(rows) + 4, dtype=torch.long)
    rows2[keep], ro2[keep], rc2[keep] = rows, ro, rc
    rows2[slots] = junk
    ro2[slots], rc2[slots] = torch.tensor([-1, 3, 0, 1]), torch.tensor([0, 1, 2, -5])
    got = ManifoldBank(rows2, ro2, rc2, 3, 2).errors(cf, o, c)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    # one-hot rows (float or int) and int vectors name the same cells
    hot = ManifoldBank(rows, torch.eye(3)[ro], torch.eye(2)[rc].int(), 3, 2).errors(cf, torch.eye(3)[o].int(),
                                                                                   torch.eye(2)[c])
    for k in want:
        assert torch.equal(hot[k], want[k]), k
    with pytest.raises(ValueError, match="columns"):
        ManifoldBank(rows, ro, rc, 3, 2).errors(cf[:, :5], o, c)


def test_abi_checks_arguments_before_any_launch():
    import ali_hip
    lib = ali_hip.load()
    assert lib.ali_group_moments(None, 4, 1, 4, None, 0, None, 1, 1, None, None, None, None, None) != 0
    assert b"ali_group_moments" in lib.ali_last_error()
    assert lib.ali_manifold_err(None, 4, 1, 4, None, None, None, None, None, None, None, None, 1, 1, None, None, 0,
                                None) != 0
    assert b"ali_manifold_err" in lib.ali_last_error()


# ------------------------------------------------------------------------------------------------ CounterfactualEval
def eval_case(dtype=torch.float64, N=24, seed=21):
    """MorphoMNIST stacks: (models {"bigan": (E, G), "vae": VAE}, clf, bank rows [N,1,28,28], owner, cls)"""
    import image_scms.mnist as pm
    from classifiers.mnist import MNISTClassifier
    from deepscm_vae.mnist import MorphoMNISTVAE
    torch.manual_seed(seed)
    E, G, vae, clf = pm.Encoder(), pm.Generator(), MorphoMNISTVAE(), MNISTClassifier()
    for m in (E, G, vae, clf):
        m.to(dtype).eval()
    g = torch.Generator().manual_seed(seed + 1)
    rows = (torch.rand(N, 1, 28, 28, generator=g) * 2 - 1).to(dtype)
    owner, cls = torch.arange(N) % 3, (torch.arange(N) // 3) % 10
    return {"bigan": (E, G), "vae": vae}, clf, rows, owner, cls


def eval_batch(B, seed, dtype=torch.float64):
    """(x, attrs, cf_attrs, owner, cls, z [2, B, 512, 1, 1])"""
    g = torch.Generator().manual_seed(100 + seed)
    x = (torch.rand(B, 1, 28, 28, generator=g) * 2 - 1).to(dtype)
    attrs = {"digit": torch.eye(10)[torch.randint(0, 10, (B,), generator=g)].to(dtype)}
    for k in ("intensity", "slant", "thickness"):
        attrs[k] = (torch.rand(B, 1, generator=g) * 2 - 1).to(dtype)
    cf_attrs = dict(attrs)
    cf_attrs["digit"] = torch.eye(10)[torch.randint(0, 10, (B,), generator=g)].to(dtype)
    owner = torch.randint(0, 3, (B,), generator=g)
    z = torch.randn(2, B, 512, 1, 1, generator=g).to(dtype)
    return x, attrs, cf_attrs, owner, cf_attrs["digit"].argmax(1), z


def scripts_body(models, clf, bank, x, attrs, cf_attrs, owner, cls, z):
    """audiomnist_cf_eval.py:78-99 / audiomnist_cf_classifier_metric.py:80-102 / mnist_bigan_score.py:79,96-98"""
    (E, G), vae = models["bigan"], models["vae"]
    with torch.no_grad():
        imgs = {"bigan_cf": G(E(x, attrs), cf_attrs), "vae_cf": vae.decoder(vae.encoder(x, attrs)[0], cf_attrs)}
        if z is not None:
            imgs["bigan_int"], imgs["vae_int"] = G(z[0], cf_attrs), vae.decoder(z[1], cf_attrs)
        out = {}
        for k, img in imgs.items():
            out[f"{k}_image"] = img
            out[f"{k}_hit_digit"] = clf(img).argmax(1) == cf_attrs["digit"].argmax(1)
            for name, v in script_loop(bank.rows, bank.owner, bank.cls, img.flatten(start_dim=1), owner, cls).items():
                out[f"{k}_{name}"] = v
    return out


def test_counterfactual_eval_on_cpu_modules_is_the_scripts_loop_body():
    from ali_hip.cfeval import CounterfactualEval, ManifoldBank
    models, clf, rows, ro, rc = eval_case()
    bank = ManifoldBank(rows, ro, rc, 3, 10)
    ev = CounterfactualEval(models, bank, {"digit": clf})
    names = [f"{m}_{k}_{c}" for m in ("bigan", "vae") for k in ("cf", "int")
             for c in ("same", "other", "ratio", "hit_digit")]
    wants = []
    for i, B in enumerate((3, 5, 2)):
        batch = eval_batch(B, i)
        got = ev.add(*batch[:5], z=batch[5])
        want = scripts_body(models, clf, bank, *batch)
        wants.append(want)
        assert set(got) == set(names) | {f"{m}_{k}_image" for m in ("bigan", "vae") for k in ("cf", "int")}
        for k in want:
            if k.endswith("_image") or "_hit_" in k:
                assert torch.equal(got[k], want[k]), k
            else:
                np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), rtol=1e-12, atol=0, err_msg=k)
    t = ev.table()
    assert list(t) == names
    for k in names:                                               # 10 rows, in the order they were added
        col = torch.cat([w[k] for w in wants]).numpy()
        assert t[k].shape == (10,)
        if "_hit_" in k:
            assert t[k].dtype == np.int64 and t[k].tolist() == col.astype(np.int64).tolist()
        else:
            np.testing.assert_allclose(t[k], col, rtol=1e-12, atol=0, equal_nan=True)
    acc = ev.accuracy()
    assert list(acc) == [k for k in names if "_hit_" in k]
    for k, v in acc.items():
        assert v == sum(int(w[k].sum()) for w in wants) / 10
    ev.reset()
    assert all(len(v) == 0 for v in ev.table().values()) and all(v == 0 for v in ev.accuracy().values())


def test_counterfactual_eval_without_interventions_bank_or_classifiers():
    from ali_hip.cfeval import CounterfactualEval, ManifoldBank
    models, clf, rows, ro, rc = eval_case()
    bank = ManifoldBank(rows, ro, rc, 3, 10)
    batch = eval_batch(4, 7)
    want = scripts_body(models, clf, bank, *batch[:5], None)
    ev = CounterfactualEval(models, bank, {"digit": clf})
    got = ev.add(*batch[:5], z=False)
    assert set(got) == set(want) and not any("_int_" in k for k in got)
    for k in want:
        if k.endswith("_image") or "_hit_" in k:
            assert torch.equal(got[k], want[k]), k
    t = ev.table()
    assert len(t["bigan_cf_ratio"]) == 4 and len(t["bigan_int_ratio"]) == 0
    acc = ev.accuracy()
    assert acc["vae_cf_hit_digit"] == int(want["vae_cf_hit_digit"].sum()) / 4 and acc["vae_int_hit_digit"] == 0
    # int labels, given explicitly, are the one-hot default; the score loops need neither a bank nor owner / cls
    sc = CounterfactualEval({"bigan": models["bigan"]}, classifiers={"digit": clf})
    got2 = sc.add(batch[0], batch[1], batch[2], labels={"digit": batch[2]["digit"].argmax(1)}, z=False)
    assert set(got2) == {"bigan_cf_image", "bigan_cf_hit_digit"}
    assert torch.equal(got2["bigan_cf_hit_digit"], want["bigan_cf_hit_digit"])
    assert list(sc.table()) == ["bigan_cf_hit_digit", "bigan_int_hit_digit"]
    # a drawn z has the models' count and the batch's shape; a bank needs the cells
    torch.manual_seed(0)
    drawn = ev.add(*batch[:5])
    assert tuple(drawn["vae_int_image"].shape) == (4, 1, 28, 28)
    with pytest.raises(ValueError, match="owner"):
        ev.add(batch[0], batch[1], batch[2])
    with pytest.raises(ValueError, match="2 models"):
        ev.add(*batch[:5], z=batch[5][:1])
