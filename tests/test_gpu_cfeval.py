"""``ali_hip.cfeval.CounterfactualEval`` on the device: the MorphoMNIST modules (``image_scms.mnist`` E / G,
``MorphoMNISTVAE``, ``MNISTClassifier``) at B = 6 with a 24-row bank of 784 columns, and the AudioMNIST stacks at d = 8,
B = 2 for D = 16384.

The executor makes the module calls the scripts make, so its images and hits are held to the direct module calls bit for
bit.  The distance columns are held to ``flow_cases.within_yardstick`` against the pairwise statement on the CPU in fp64
(yardstick: the same in fp32) EVALUATED ON THE DEVICE-PRODUCED IMAGES copied to the host, so the conv stacks' own
deviation does not enter."""
import copy

import pytest
import torch

from flow_cases import within_yardstick
from test_cfeval_cpu import eval_case

pytestmark = pytest.mark.gpu


def _batch(B, seed):
    """(x, attrs, cf_attrs, owner, cls, z) on the device; counterfactual digits among the bank's classes 0 .. 7"""
    g = torch.Generator().manual_seed(300 + seed)
    x = torch.rand(B, 1, 28, 28, generator=g) * 2 - 1
    attrs = {"digit": torch.eye(10)[torch.randint(0, 10, (B,), generator=g)]}
    for k in ("intensity", "slant", "thickness"):
        attrs[k] = torch.rand(B, 1, generator=g) * 2 - 1
    cf_attrs = dict(attrs)
    cf_attrs["digit"] = torch.eye(10)[torch.randint(0, 8, (B,), generator=g)]
    owner = torch.randint(0, 3, (B,), generator=g)
    z = torch.randn(2, B, 512, 1, 1, generator=g)
    dev = lambda d: {k: v.cuda() for k, v in d.items()}       # noqa: E731
    return x.cuda(), dev(attrs), dev(cf_attrs), owner.cuda(), cf_attrs["digit"].argmax(1).cuda(), z.cuda()


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if a.is_floating_point():
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0)), what
    else:
        assert torch.equal(a, b), what


def _direct(models, clf, batch):
    """the scripts' module calls, one by one"""
    x, attrs, cf_attrs, _, _, z = batch
    (E, G), vae = models["bigan"], models["vae"]
    with torch.no_grad():
        imgs = {"bigan_cf": G(E(x, attrs), cf_attrs), "bigan_int": G(z[0], cf_attrs),
                "vae_cf": vae.decoder(vae.encoder(x, attrs)[0], cf_attrs), "vae_int": vae.decoder(z[1], cf_attrs)}
        hits = {k: clf(v).argmax(1) == cf_attrs["digit"].argmax(1) for k, v in imgs.items()}
    return imgs, hits


def _check_distances(name, got, img, rows, ro, rc, O, C, owner, cls):
    from ali_hip.cfeval import ManifoldBank
    host = img.detach().cpu().reshape(img.shape[0], -1)
    worst = 0.0
    stmt = {dt: ManifoldBank(rows.to(dt), ro, rc, O, C).errors(host.to(dt), owner.cpu(), cls.cpu())
            for dt in (torch.float64, torch.float32)}
    for k in ("same", "other", "ratio"):
        worst = max(worst, within_yardstick(f"{name}_{k}", got[f"{name}_{k}"], stmt[torch.float64][k],
                                            stmt[torch.float32][k]))
    return worst


def test_mnist_executor_against_direct_module_calls_and_the_cpu_statement():
    from ali_hip.cfeval import CounterfactualEval, ManifoldBank
    models, clf, rows, ro, rc = eval_case(torch.float32)
    md = {"bigan": tuple(copy.deepcopy(m).cuda() for m in models["bigan"]), "vae": copy.deepcopy(models["vae"]).cuda()}
    clf_d = copy.deepcopy(clf).cuda()
    bank = ManifoldBank(rows.cuda(), ro.cuda(), rc.cuda(), 3, 10)
    batches = [_batch(6, i) for i in range(3)]
    outs, worst = {}, 0.0
    for capture in (False, True):
        ev = CounterfactualEval(md, bank, {"digit": clf_d}, capture=capture)
        outs[capture] = [ev.add(*b[:5], z=b[5]) for b in batches]
        if not capture:
            continue
        assert len(ev._graphs) == 1                                  # three batches, one signature
        for b, got in zip(batches, outs[True]):
            imgs, hits = _direct(md, clf_d, b)
            for k in imgs:
                assert torch.equal(got[f"{k}_image"], imgs[k]), k    # the module calls' images, bit for bit
                assert torch.equal(got[f"{k}_hit_digit"], hits[k]), k
                worst = max(worst, _check_distances(k, got, imgs[k], rows.reshape(24, -1), ro, rc, 3, 10, b[3], b[4]))
        # counters, accuracy and the table agree with the returned columns
        acc, t = ev.accuracy(), ev.table()
        for k in acc:
            col = torch.cat([o[k] for o in outs[True]])
            assert acc[k] == int(col.sum()) / 18 and t[k].tolist() == col.long().tolist(), k
        for k in ("bigan_cf_ratio", "vae_int_same"):
            assert t[k].tolist() == torch.cat([o[k] for o in outs[True]]).tolist(), k
        # a second signature gets its own graph
        ev.add(*[v[:4] if torch.is_tensor(v) else {k: u[:4] for k, u in v.items()} for v in batches[0][:5]],
               z=batches[0][5][:, :4])
        assert len(ev._graphs) == 2 and len(ev.table()["vae_cf_same"]) == 22
        # what add returned stays the caller's: a replay on other data does not touch it
        held = {k: v.clone() for k, v in outs[True][2].items()}
        other = ev.add(*batches[0][:5], z=batches[0][5])
        assert len(ev._graphs) == 2
        for k in held:
            _same_bits(outs[True][2][k], held[k], k)
            _same_bits(other[k], outs[True][0][k], k)
        # an in-place weight update drops the graphs, and the next add reflects it: the BiGAN generator's last bias
        # moves its images and leaves the VAE's alone
        with torch.no_grad():
            md["bigan"][1].layers[-2].bias.add_(0.25)
        again = ev.add(*batches[0][:5], z=batches[0][5])
        assert len(ev._graphs) == 1
        assert not torch.equal(again["bigan_cf_image"], other["bigan_cf_image"])
        assert bool((again["bigan_int_same"] != other["bigan_int_same"]).all())
        for k in again:
            if k.startswith("vae_"):
                _same_bits(again[k], other[k], k)
        imgs, _ = _direct(md, clf_d, batches[0])
        assert torch.equal(again["bigan_cf_image"], imgs["bigan_cf"])
        with torch.no_grad():
            md["bigan"][1].layers[-2].bias.sub_(0.25)
    for a, b in zip(outs[False], outs[True]):                        # captured and eager: the same bits
        assert set(a) == set(b)
        for k in a:
            _same_bits(a[k], b[k], k)
    print(f"cfeval mnist executor: worst yardstick ratio {worst:.3g}")


def test_audio_executor_at_16384_columns():
    from ali_hip.cfeval import CounterfactualEval, ManifoldBank
    from test_gpu_modules import paired_models, to_dev
    _, (E, G, _), images, c, z = paired_models("audio", d=8, B=2)
    E.eval(), G.eval()
    g = torch.Generator().manual_seed(8)
    rows = torch.clip(torch.randn(6, 128, 128, generator=g), -3, 3) / 3
    ro, rc = torch.tensor([0, 1, 0, 1, 1, 0]), torch.tensor([3, 3, 3, 3, 5, 3])
    bank = ManifoldBank(rows.cuda(), ro.cuda(), rc.cuda(), 2, 10)
    cf_c = dict(c)
    cf_c["digit"] = torch.eye(10)[torch.tensor([3, 3])]
    x, cd, cfd, zd = images.cuda(), to_dev(c), to_dev(cf_c), z.reshape(1, 2, 512, 1, 1).cuda()
    owner = torch.tensor([0, 1], dtype=torch.int32).cuda()
    outs = []
    for capture in (False, True):
        ev = CounterfactualEval({"bigan": (E, G)}, bank, capture=capture)
        first = ev.add(x, cd, cfd, owner, 3, z=zd)
        outs.append(ev.add(x, cd, cfd, owner, 3, z=zd))                 # (captured: a pure replay)
        for k in first:
            _same_bits(first[k], outs[-1][k], k)
    for k in outs[0]:
        _same_bits(outs[0][k], outs[1][k], k)
    with torch.no_grad():
        imgs = {"bigan_cf": G(E(x, cd), cfd), "bigan_int": G(zd[0], cfd)}
    worst = 0.0
    cls = torch.full((2,), 3)
    for k, img in imgs.items():
        assert torch.equal(outs[1][f"{k}_image"], img), k
        worst = max(worst, _check_distances(k, outs[1], img, rows.reshape(6, -1), ro, rc, 2, 10, owner.long(), cls))
    assert sorted(ev.table()) == sorted(f"bigan_{k}_{c}" for k in ("cf", "int") for c in ("same", "other", "ratio"))
    print(f"cfeval audio executor: worst yardstick ratio {worst:.3g}")
