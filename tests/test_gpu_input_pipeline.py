"""Device-side input pipeline on the GPU: ``ali_normal_fill`` against its host definition, ``ali_batch_gather``
against ``_scale_batch`` + ``MnistFamily.conditioning``, and the stepper / training-loop entry points built on them
against the host pipeline fed the same rows and the same latents -- bit for bit."""
import numpy as np
import pytest
import torch

import ali_oracle as orc

pytestmark = pytest.mark.gpu


def _ops():
    import ali_hip
    from ali_hip import ops
    ali_hip.load()
    return ops


def _counter(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


def _fill(seed, counter, n, offset=0):
    return _ops().normal_fill(seed, torch.empty(n, device="cuda"), dev_counter=_counter(counter), offset=offset)


# ----------------------------------------------------------------------------- ali_normal_fill
@pytest.mark.parametrize("seed,counter", [(0x5EED, 0), (12345, 7)])
def test_normal_fill_vs_host_reference(seed, counter):
    """The integers behind every draw are exact on both sides, so the device may differ from the fp64 reference only by
    the rounding of its fp32 log / sqrt / sin / cos.  Bound: 4 x the largest deviation a numpy-float32 evaluation of the
    same formula shows from the fp64 reference (4: device transcendentals are a few ulp, not correctly rounded)."""
    from ali_hip.source import latent_bits, normal_reference
    n = 512 * 512
    ref = normal_reference(seed, counter, n).numpy()
    k1, k2, odd = latent_bits(seed, counter, n)
    u1 = k1.astype(np.float32) * np.float32(2.0 ** -24)
    u2 = k2.astype(np.float32) * np.float32(2.0 ** -24)
    rad = np.sqrt(np.float32(-2.0) * np.log(u1))
    ang = np.float32(2.0 * np.pi) * u2
    f32 = rad * np.where(odd, np.sin(ang), np.cos(ang))
    assert f32.dtype == np.float32
    bound = 4.0 * np.abs(f32.astype(np.float64) - ref).max()
    got = _fill(seed, counter, n).cpu().numpy().astype(np.float64)
    dev = np.abs(got - ref).max()
    print(f"normal_fill seed {seed:#x} counter {counter}: device max |dev| {dev:.3e}, numpy-f32 max |dev| {bound / 4:.3e}")
    assert dev <= bound, (dev, bound)


@pytest.mark.parametrize("n", [1, 3, 4097, 512 * 512])
def test_normal_fill_is_reproducible_and_independent_of_the_split(n):
    ops = _ops()
    a, b = _fill(77, 3, n), _fill(77, 3, n)
    assert torch.equal(a, b)
    assert bool(torch.isfinite(a).all())
    assert not torch.equal(a, _fill(77, 4, n)) and not torch.equal(a, _fill(78, 3, n))
    if n > 1:
        k = 1 if n < 8 else 1333                      # odd: the second launch starts in the middle of a Box-Muller pair,
        out = torch.full((n,), float("nan"), device="cuda")       # at an address that is not 16-byte aligned
        ops.normal_fill(77, out[:k], dev_counter=_counter(3))
        ops.normal_fill(77, out[k:], dev_counter=_counter(3), offset=k)
        assert torch.equal(out, a)
    # a launch writes its n elements and nothing else
    buf = torch.full((n + 9,), 7.0, device="cuda")
    ops.normal_fill(77, buf[5:5 + n], dev_counter=_counter(3))
    assert torch.equal(buf[5:5 + n], a) and bool((buf[:5] == 7).all()) and bool((buf[5 + n:] == 7).all())


def test_normal_fill_without_counter_is_counter_zero():
    ops = _ops()
    assert torch.equal(ops.normal_fill(5, torch.empty(1000, device="cuda")), _fill(5, 0, 1000))


def test_normal_fill_in_a_captured_graph_follows_the_counter():
    ops = _ops()
    n = 512 * 512
    ctr = _counter(0)
    out = torch.zeros(n, device="cuda")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        ops.normal_fill(0xABC, out, dev_counter=ctr)
    torch.cuda.synchronize()
    seen = []
    for t in (0, 1, 6):
        ctr.fill_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, _fill(0xABC, t, n)), t
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ----------------------------------------------------------------------------- ali_batch_gather
def _dataset(n, seed=3, soft=True):
    x, a = orc.synth_morphomnist(n, seed=seed)
    if soft:                # soft "one-hot" rows, some with tied maxima: torch.argmax takes the first
        g = torch.Generator().manual_seed(seed)
        soft_rows = torch.rand(n // 4, 10, generator=g)
        soft_rows[::2, 7] = soft_rows[::2].max(dim=1).values
        soft_rows[::2, 2] = soft_rows[::2, 7]
        a["digit"][: n // 4] = soft_rows
    return x, a


def _host_batch(x, a, rows, device="cuda"):
    import image_scms.mnist as pm
    stats = {k: (v.min(dim=0).values, v.max(dim=0).values) for k, v in a.items() if k != "digit"}
    return pm._scale_batch(x[rows], {k: v[rows] for k, v in a.items()}, stats, device)


@pytest.mark.parametrize("kind", ["uint8", "fp32", "fp32_fractional"])
@pytest.mark.parametrize("B", [1, 37, 64, 512])
def test_batch_gather_vs_scale_batch_and_conditioning(kind, B):
    from ali_hip.source import DeviceDataset
    from ali_hip.step import MnistFamily
    _ops()
    n = 300
    x, a = _dataset(n)
    if kind == "uint8":
        x = x.to(torch.uint8)
    elif kind == "fp32_fractional":
        x = x * 0.731
    src = DeviceDataset(x, a, "cuda")
    assert src.images.dtype == (torch.uint8 if kind == "uint8" else torch.float32)
    g = torch.Generator().manual_seed(B)
    rows = torch.randint(0, n, (B,), generator=g)
    if B > 1:
        rows[1] = rows[0]                           # a repeated index
        rows[-1] = n - 1
    images, onehot, idx, cont = src.gather(rows.cuda())
    ref_images, c = _host_batch(x, a, rows)
    ref_idx, ref_cont, ref_onehots = MnistFamily.conditioning(c)
    assert images.shape == ref_images.shape == (B, 1, 28, 28)
    assert torch.equal(images, ref_images)
    assert torch.equal(onehot, ref_onehots[0])
    assert idx.dtype == torch.int32 and torch.equal(idx, ref_idx)
    assert torch.equal(idx.reshape(-1).long().cpu(), a["digit"][rows].argmax(1))
    assert torch.equal(cont, ref_cont)


def test_batch_gather_rows_that_are_not_a_multiple_of_four_pixels():
    """the one-pixel-per-lane form (H*W % 4 != 0) gives what the vector form gives"""
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    n, hw = 50, 27
    for dt in (torch.uint8, torch.float32):
        x = torch.randint(0, 256, (n, hw), generator=g).to(dt).cuda()
        attrs = torch.rand(n, 12, generator=g).cuda()
        lo, hi = attrs[:, 10:].min(dim=0).values.contiguous(), attrs[:, 10:].max(dim=0).values.contiguous()
        rows = torch.randint(0, n, (33,), generator=g).cuda()
        images, onehot, idx, cont = ops.batch_gather(x, attrs, 10, rows, lo, hi)
        assert torch.equal(images, 2 * x[rows].float() / 255 - 1)
        assert torch.equal(onehot, attrs[rows, :10]) and torch.equal(idx.reshape(-1).long(), attrs[rows, :10].argmax(1))
        a_cpu, lo_c, hi_c = attrs[rows, 10:].cpu(), lo.cpu(), hi.cpu()
        assert torch.equal(cont.cpu(), 2 * (a_cpu - lo_c) / (hi_c - lo_c) - 1)


def test_device_dataset_batches_and_validation():
    from ali_hip.source import DeviceDataset
    x, a = _dataset(20, soft=False)
    src = DeviceDataset(x, a, "cuda", batch_size=8)
    assert src.keys == ["intensity", "slant", "thickness"] and len(src) == 20
    perm = np.random.RandomState(0).permutation(20)
    src.set_epoch(perm)
    assert src.n_batches == 3
    assert [src.batch(i).numel() for i in range(3)] == [8, 8, 4]
    assert torch.equal(torch.cat([src.batch(i) for i in range(3)]).cpu(), torch.from_numpy(perm))
    with pytest.raises(ValueError):
        src.set_epoch(np.array([0, 20]))
    with pytest.raises(IndexError):
        src.batch(3)
    with pytest.raises(ValueError):
        DeviceDataset(x, a, "cpu")


# ----------------------------------------------------------------------------- the stepper
def _mnist_models(seed=5):
    import image_scms.mnist as pm
    torch.manual_seed(seed)
    E, G, D = pm.Encoder(), pm.Generator(), pm.Discriminator()
    for i, m in enumerate((E, G, D)):
        m.apply(pm.init_weights)
        orc.rescale_for_test_(m, 0.01, bias_seed=7 + i)
    return E.cuda(), G.cuda(), D.cuda()


def _assert_same_state(sa, sb, what):
    """every parameter, buffer and Adam moment of two steppers, bit for bit"""
    for ma, mb, name in ((sa.E, sb.E, "E"), (sa.G, sb.G, "G"), (sa.D, sb.D, "D")):
        da, db = ma.state_dict(), mb.state_dict()
        assert list(da) == list(db)
        for k in da:
            assert torch.equal(da[k], db[k]), (what, name, k)
    for ga, gb, name in ((sa.opt_eg, sb.opt_eg, "opt_eg"), (sa.opt_d, sb.opt_d, "opt_d")):
        assert torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v), (what, name)
        assert int(ga.step_t) == int(gb.step_t), (what, name)
    assert int(sa.iter_t) == int(sb.iter_t), what


def _assert_same_result(ra, rb, what):
    assert set(ra) == set(rb), (what, set(ra), set(rb))
    for k in ra:
        assert torch.equal(ra[k], rb[k]), (what, k, float(ra[k]), float(rb[k]))
        assert bool(torch.isfinite(ra[k]).all()), (what, k)


@pytest.mark.parametrize("kind", ["uint8", "fp32"])
@pytest.mark.parametrize("capture", [False, True])
def test_step_indexed_equals_step_on_the_same_rows_and_latents(capture, kind):
    """Four consecutive iterations (one with do_eg=False, the last on a ragged batch) through ``step_indexed`` and
    through ``step`` fed ``_scale_batch`` of the same rows and ``normal_fill`` with the same key."""
    import ali_hip
    from ali_hip.source import DeviceDataset
    from ali_hip.step import AliStepper
    ops = _ops()
    n, bs, z_seed = 200, 64, 4242
    x, a = _dataset(n, seed=6)
    if kind == "uint8":
        x = x.to(torch.uint8)
    perm = np.random.RandomState(3).permutation(n)
    schedule = [True, False, True, True]
    src = DeviceDataset(x, a, "cuda", batch_size=bs).set_epoch(perm)
    assert src.n_batches == 4 and src.batch(3).numel() == n - 3 * bs

    ali_hip.manual_seed(9)
    sa = AliStepper(*_mnist_models(), capture=capture, z_seed=z_seed)
    res_a = []
    for i, do_eg in enumerate(schedule):
        r = sa.step_indexed(src, src.batch(i), do_eg=do_eg)
        res_a.append({k: v.clone() for k, v in r.items()})
    assert "z_seed" in sa.state_dict()

    ali_hip.manual_seed(9)
    sb = AliStepper(*_mnist_models(), capture=capture, z_seed=z_seed)
    assert "z_seed" not in sb.state_dict()          # host latents: today's checkpoint keys
    for i, do_eg in enumerate(schedule):
        rows = torch.from_numpy(perm[i * bs:(i + 1) * bs])
        images, c = _host_batch(x, a, rows)
        z = ops.normal_fill(z_seed, torch.empty(len(rows), 512, device="cuda"), dev_counter=sb.iter_t)
        r = sb.step(images, c, z.reshape(-1, 512, 1, 1), do_eg=do_eg)
        _assert_same_result(res_a[i], r, f"iteration {i}")
    _assert_same_state(sa, sb, f"capture={capture} {kind}")
    if capture:
        assert any(k[-1] == "indexed" for k in sa._graph), "step_indexed did not replay a graph"
        ent = next(v[0] for k, v in sa._graph.items() if k[-1] == "indexed")
        assert len(ent.inputs) == 1 and ent.inputs[0].dtype == torch.int64      # the index slice is all a replay loads


@pytest.mark.parametrize("capture", [False, True])
def test_step_without_z_draws_the_documented_latents(capture):
    import ali_hip
    from ali_hip.step import AliStepper
    ops = _ops()
    x, a = _dataset(64, seed=8)
    ali_hip.manual_seed(2)
    sa = AliStepper(*_mnist_models(), capture=capture)          # default z_seed
    ali_hip.manual_seed(2)
    sb = AliStepper(*_mnist_models(), capture=capture)
    from ali_hip.source import DEFAULT_Z_SEED
    assert sa.latent_seed == DEFAULT_Z_SEED
    for i in range(3):
        rows = torch.arange(i * 16, i * 16 + 32)
        images, c = _host_batch(x, a, rows)
        ra = {k: v.clone() for k, v in sa.step(images, c).items()}
        z = ops.normal_fill(DEFAULT_Z_SEED, torch.empty(32, 512, device="cuda"), dev_counter=sb.iter_t)
        _assert_same_result(ra, sb.step(images, c, z), f"iteration {i}")
    _assert_same_state(sa, sb, f"capture={capture}")


def test_device_pipeline_refuses_pipeline_reduce_and_ahead():
    from ali_hip.source import DeviceDataset
    from ali_hip.step import AliStepper
    _ops()
    x, a = _dataset(32, soft=False)
    src = DeviceDataset(x, a, "cuda", batch_size=16).set_epoch(np.arange(32))
    images, c = _host_batch(x, a, torch.arange(16))
    st = AliStepper(*_mnist_models(), pipeline_reduce=True)
    with pytest.raises(ValueError):
        st.step(images, c)
    with pytest.raises(ValueError):
        st.step_indexed(src, src.batch(0))
    st = AliStepper(*_mnist_models())
    with pytest.raises(ValueError):
        st.step(images, c, None, ahead=(images, c, None))
    with pytest.raises(ValueError):
        st.step_indexed(src, src.batch(0).int())
    assert "z_seed" not in st.state_dict()          # a refused call leaves the checkpoint keys alone


def _four_indexed_iterations(st, src):
    out = []
    for i, do_eg in enumerate([True, False, True, True]):
        out.append({k: v.clone() for k, v in st.step_indexed(src, src.batch(i), do_eg=do_eg).items()})
    return out


def test_segmented_replay_with_the_device_pipeline_equals_eager():
    """the data-parallel replay (one HIP graph per segment) on one rank, gather and draw inside the first segment's graph"""
    import ali_hip
    from ali_hip.source import DeviceDataset
    from ali_hip.step import AliStepper
    _ops()
    n, bs = 200, 64
    x, a = _dataset(n, seed=6)
    src = DeviceDataset(x.to(torch.uint8), a, "cuda", batch_size=bs).set_epoch(np.random.RandomState(3).permutation(n))
    ali_hip.manual_seed(9)
    eager = AliStepper(*_mnist_models(), capture=False, z_seed=11)
    res_e = _four_indexed_iterations(eager, src)
    ali_hip.manual_seed(9)
    seg = AliStepper(*_mnist_models(), capture=True, z_seed=11)
    seg.segmented = True
    for i, (re, rs) in enumerate(zip(res_e, _four_indexed_iterations(seg, src))):
        _assert_same_result(re, rs, f"iteration {i}")
    _assert_same_state(eager, seg, "segmented")
    assert any(k[0] == "seg" and k[-1] == "indexed" for k in seg._graph), "the segmented replay did not run"


@pytest.mark.parametrize("capture", [False, True])
def test_device_latents_under_a_process_group_and_rank_mixing(capture):
    """A 1-rank RCCL group with z=None: every collective of the schedule is issued around the in-iteration draw, and
    rank 0 draws with z_seed itself, so the result equals the group-less stepper's.  A stepper that is rank 3 draws
    the stream of ``rank_seed(z_seed, 3)``: another one, and the one ``step`` reproduces when handed those latents."""
    import os
    import torch.distributed as dist
    import ali_hip
    from ali_hip.source import rank_seed
    from ali_hip.step import AliStepper
    ops = _ops()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        x, a = _dataset(64, seed=8)
        batches = [_host_batch(x, a, torch.arange(i * 16, i * 16 + 32)) for i in range(3)]
        ali_hip.manual_seed(2)
        plain = AliStepper(*_mnist_models(), capture=capture, z_seed=321)
        ali_hip.manual_seed(2)
        grouped = AliStepper(*_mnist_models(), capture=capture, z_seed=321, process_group=dist.group.WORLD)
        assert grouped.dist and grouped.rank == 0 and grouped.latent_seed == 321
        for i, (images, c) in enumerate(batches):
            rp = {k: v.clone() for k, v in plain.step(images, c).items()}
            _assert_same_result(rp, grouped.step(images, c), f"iteration {i}")
        _assert_same_state(plain, grouped, "1-rank group")

        ali_hip.manual_seed(2)
        r3 = AliStepper(*_mnist_models(), capture=capture, z_seed=321, process_group=dist.group.WORLD)
        r3.rank = 3                                       # what rank 3 of a larger group would draw
        assert r3.latent_seed == rank_seed(321, 3) != 321
        ali_hip.manual_seed(2)
        fed = AliStepper(*_mnist_models(), capture=capture)
        for i, (images, c) in enumerate(batches):
            r = {k: v.clone() for k, v in r3.step(images, c).items()}
            z = ops.normal_fill(rank_seed(321, 3), torch.empty(32, 512, device="cuda"), dev_counter=fed.iter_t)
            _assert_same_result(r, fed.step(images, c, z), f"rank 3, iteration {i}")
        _assert_same_state(r3, fed, "rank 3")
        assert not torch.equal(r3.opt_eg.flat, plain.opt_eg.flat)
    finally:
        if created:
            dist.destroy_process_group()


# ----------------------------------------------------------------------------- mnist.train
def _train_device(x, a, n_epochs, bs, z_seed, **kw):
    import ali_hip
    import image_scms.mnist as pm
    ali_hip.manual_seed(4)
    torch.manual_seed(4)
    np.random.seed(4)
    return pm.train(x, a, n_epochs=n_epochs, device="cuda", save_images_every=None, batch_size=bs,
                    input_pipeline="device", z_seed=z_seed, **kw)


def _weights(*mods):
    return [v.detach().clone() for m in mods for v in m.state_dict().values()]


def test_mnist_train_device_pipeline_equals_hand_written_loop():
    """N = 200, bs = 64, two epochs of ``mnist.train(input_pipeline="device")`` against the statements of ``train``
    written out over the same permutations with ``stepper.step`` on host-made batches and ``normal_fill`` latents;
    a second run is identical; everything is finite."""
    import ali_hip
    import image_scms.mnist as pm
    from ali_hip.step import AliStepper
    ops = _ops()
    n, bs, z_seed = 200, 64, 31337
    x, a = orc.synth_morphomnist(n, seed=5)
    x = x.to(torch.uint8)
    E, G, D, oD, oE = _train_device(x, a, 2, bs, z_seed)
    got = _weights(E, G, D)
    assert all(bool(torch.isfinite(t).all()) for t in got if t.is_floating_point())
    assert oD.state_dict()["step"] == 16 and oE.state_dict()["step"] == 8

    E2, G2, D2, _, _ = _train_device(x, a, 2, bs, z_seed)
    assert all(torch.equal(p, q) for p, q in zip(got, _weights(E2, G2, D2))), "two runs differ"

    ali_hip.manual_seed(4)
    torch.manual_seed(4)
    np.random.seed(4)
    Eh, Gh, Dh = pm.Encoder().to("cuda"), pm.Generator().to("cuda"), pm.Discriminator().to("cuda")
    for m in (Eh, Gh, Dh):
        m.apply(pm.init_weights)
    st = AliStepper(Eh, Gh, Dh, lr=1e-4, betas=(0.5, 0.999), capture=True)
    for _ in range(2):
        for m in (Dh, Eh, Gh):
            m.train()
        perm = torch.from_numpy(np.random.permutation(n))
        for i in range(0, n, bs):
            images, c = _host_batch(x, a, perm[i:i + bs])
            z = ops.normal_fill(z_seed, torch.empty(images.shape[0], 512, device="cuda"), dev_counter=st.iter_t)
            st.step(images, c, z)
    hand = _weights(Eh, Gh, Dh)
    assert len(hand) == len(got)
    for k, (p, q) in enumerate(zip(got, hand)):
        assert torch.equal(p, q), f"tensor {k} differs from the hand-written loop"
    assert torch.equal(oE.m, st.opt_eg.m) and torch.equal(oD.v, st.opt_d.v)
    other = _weights(*_train_device(x, a, 2, bs, z_seed + 1)[:3])
    assert not all(torch.equal(p, q) for p, q in zip(got, other)), "z_seed has no effect"


def test_checkpoint_resume_continues_the_latent_stream(tmp_path):
    """A checkpoint after epoch 1, loaded into a fresh stepper (constructed with another z_seed) and run for epoch 2,
    equals the uninterrupted two epochs bit for bit: the checkpoint carries z_seed and the iteration counter that
    key the latents."""
    import ali_hip
    from ali_hip.source import DeviceDataset
    from ali_hip.step import AliStepper
    _ops()
    n, bs = 200, 64
    x, a = orc.synth_morphomnist(n, seed=7)
    x = x.to(torch.uint8)
    perms = [np.random.RandomState(s).permutation(n) for s in (1, 2)]
    src = DeviceDataset(x, a, "cuda", batch_size=bs)

    def epoch(st, perm):
        src.set_epoch(perm)
        for i in range(src.n_batches):
            st.step_indexed(src, src.batch(i))

    ali_hip.manual_seed(6)
    whole = AliStepper(*_mnist_models(), capture=True, z_seed=2024)
    epoch(whole, perms[0])
    epoch(whole, perms[1])

    ali_hip.manual_seed(6)
    first = AliStepper(*_mnist_models(), capture=True, z_seed=2024)
    epoch(first, perms[0])
    ck = tmp_path / "ck.tar"
    torch.save(first.state_dict(), ck)
    sd = torch.load(ck)
    assert sd["z_seed"] == 2024 and sd["iteration"] == 4

    resumed = AliStepper(*_mnist_models(seed=99), capture=True, z_seed=1)
    resumed.load_state_dict(sd)
    assert resumed.z_seed == 2024 and "z_seed" in resumed.state_dict()
    epoch(resumed, perms[1])
    _assert_same_state(whole, resumed, "resumed")

    old = {k: v for k, v in sd.items() if k != "z_seed"}           # a checkpoint of a host-latent run loads as before
    st = AliStepper(*_mnist_models(seed=98), z_seed=5)
    st.load_state_dict(old)
    assert st.z_seed == 5 and "z_seed" not in st.state_dict()


# ----------------------------------------------------------------------------- train_on_stream
def test_train_on_stream_device_latents_equal_step_with_reconstructed_z():
    import ali_hip
    import image_scms.audio_mnist as pm
    from ali_hip.step import AliStepper
    from image_scms import _spect
    ops = _ops()
    d, B, z_seed = 8, 4, 808
    batches = []
    for s in (1, 2):
        images, attrs, _ = orc.synth_spect_batch("audio", B, seed=s)
        batches.append({"audio": images.reshape(B, 128, 128), **attrs})
    keys = tuple(k for k in batches[0] if k != "audio")

    def models():
        torch.manual_seed(12)
        E, G, D = pm.Encoder(d), pm.Generator(d), pm.Discriminator(d)
        for m in (E, G, D):
            m.apply(pm.init_weights)
        return E.cuda(), G.cuda(), D.cuda()

    ali_hip.manual_seed(3)
    E, G, D = models()
    state = torch.get_rng_state()
    _spect.train_on_stream(E, G, D, lambda: iter(batches), n_epochs=1, device="cuda", attr_keys=keys,
                           z_source="device", z_seed=z_seed)
    assert torch.equal(state, torch.get_rng_state()), "the device latents must leave torch's host generator alone"

    ali_hip.manual_seed(3)
    E2, G2, D2 = models()
    st = AliStepper(E2, G2, D2, lr=1e-4, betas=(0.5, 0.9), capture=True)
    for m in (D2, E2, G2):
        m.train()
    for b in batches:
        images = b["audio"].reshape(-1, 1, 128, 128).float().cuda()
        c = {k: b[k].clone().float().cuda() for k in keys}
        z = ops.normal_fill(z_seed, torch.empty(B, 512, device="cuda"), dev_counter=st.iter_t)
        st.step(images, c, z)
    for p, q in zip(_weights(E, G, D), _weights(E2, G2, D2)):
        assert torch.equal(p, q)
    assert all(bool(torch.isfinite(t).all()) for t in _weights(E, G, D) if t.is_floating_point())
