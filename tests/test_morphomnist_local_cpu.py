"""The statement of the Morpho-MNIST local perturbations on the host: ``morphomnist.skeleton`` (neighbours, erase, the
order of the two prunes, direction, the sampler's draws) and the second half of ``morphomnist.perturb`` (the digital
line, ``Swelling``, ``Fracture``, ``local_image``), and ``ali_hip.morpho.MorphoLocal`` on CPU tensors."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import local_cases as lc
import morpho_cases as mc
from ali_hip import rng
from ali_hip.morpho import MorphoLocal, unpack_bits
from morphomnist import perturb as p
from morphomnist import skeleton as sk
from morphomnist.morpho import ImageMorphology, _components


class _Morph:
    def __init__(self, skeleton, scale=1, binary=None, d2=None, thickness=2.0):
        self.skeleton, self.scale = skeleton, scale
        self.binary_image = skeleton if binary is None else binary
        self.squared_distance, self.mean_thickness = d2, np.float64(thickness)


def _disk(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return x * x + y * y <= r * r


def test_num_neighbours_against_convolve():
    for name, s in lc.skeletons().items():
        want = ndimage.convolve(s.astype(int), np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]]), mode="constant") * s
        assert np.array_equal(sk.num_neighbours(s), want), name


@pytest.mark.parametrize("r", [0, 1, 3, 8])
def test_erase_against_dilation_by_the_exact_disk(r):
    g = np.random.default_rng(r)
    skel = g.random((20, 45)) < 0.5
    seeds = np.zeros_like(skel)
    seeds[[0, 0, 19, 19, 7, 12], [0, 44, 0, 44, 31, 32]] = True      # the four corners and the word boundary
    want = skel & ~ndimage.binary_dilation(seeds, _disk(r))
    assert np.array_equal(sk.erase(skel, seeds, r), want)
    assert np.array_equal(sk.erase(skel, np.zeros_like(skel), r), skel)


def test_the_two_prunes_run_in_order_on_a_tee():
    """the stem's stump left by the first erase is a tip of the pruned skeleton, not a fork: the fork count is taken
    after the tips are pruned, on what is left"""
    s = lc.tee()
    nn = sk.num_neighbours(s)
    assert (nn == 1).sum() == 3 and (nn == 3).sum() == 3             # the junction and its two neighbours on the bar
    first = sk.erase(s, nn == 1, 4)
    want = sk.erase(first, sk.num_neighbours(first) == 3, 2)
    assert np.array_equal(sk.candidates(s, 2, prune_tips=2, prune_forks=1), want)
    other = sk.erase(sk.erase(s, nn == 3, 2), nn == 1, 4)            # both seeds from the unpruned skeleton
    short = np.zeros_like(s)                                         # a stem so short that pruning its tip removes the fork
    short[4, 20:60] = True
    short[5:8, 33] = True
    a = sk.candidates(short, 1, prune_tips=4, prune_forks=3)
    b = sk.erase(sk.erase(short, sk.num_neighbours(short) == 1, 4), sk.num_neighbours(short) == 3, 3)
    assert a.sum() > b.sum() and np.array_equal(want, other)         # (on the long stem the order does not matter)


def test_plus_ring_one_and_empty():
    cases = lc.skeletons()
    nn = sk.num_neighbours(cases["plus"])
    assert nn[11, 32] == 4 and (nn == 3).sum() == 0 and (nn == 1).sum() == 4     # the centre is no fork
    assert np.array_equal(sk.candidates(cases["plus"], 1, None, 5), cases["plus"])
    ring = cases["ring"]
    assert (sk.num_neighbours(ring)[ring] == 2).all()                # no tips, no forks: nothing is pruned
    assert np.array_equal(sk.candidates(ring, 4, 2, 2), ring)
    one = cases["one"]
    assert tuple(sk.LocationSampler().sample(_Morph(one))) == (12, 32)
    assert sk.num_neighbours(one).sum() == 0 and sk.direction(sk.window_sums(one, 12, 32, 4)) == (1.0, 0.0)
    with pytest.raises(ValueError, match="Overpruned skeleton"):
        sk.LocationSampler().sample(_Morph(cases["none"]))
    with pytest.raises(ValueError, match="Overpruned skeleton"):
        sk.LocationSampler(2, 2).sample(_Morph(cases["run"], scale=40))


def test_direction_against_arctan2():
    g = np.random.default_rng(5)
    for trial in range(200):
        r = int(g.integers(1, 9))
        win = g.random((2 * r + 1, 2 * r + 1)) < g.uniform(0.1, 0.9)
        if win.sum() < 2:
            continue
        big = np.zeros((40, 40), dtype=bool)
        big[10:10 + 2 * r + 1, 12:12 + 2 * r + 1] = win
        sums = sk.window_sums(big, 10 + r, 12 + r, r)
        ys, xs = np.nonzero(win)
        assert sums == (len(ys), xs.sum(), ys.sum(), (xs * xs).sum(), (xs * ys).sum(), (ys * ys).sum())
        n = len(ys)
        u20, u02 = (xs * xs).sum() / n - (xs.sum() / n) ** 2, (ys * ys).sum() / n - (ys.sum() / n) ** 2
        u11 = (xs * ys).sum() / n - xs.sum() * ys.sum() / n ** 2
        c, s = sk.direction(sums)
        if np.hypot(2 * u11, u20 - u02) < 1e-9:
            continue
        want = 0.5 * np.arctan2(2 * u11, u20 - u02)
        got = np.arctan2(s, c)
        assert abs(got - want) <= 1e-12 or abs(abs(got - want) - np.pi) <= 1e-12, (trial, got, want)
        assert abs(sk.get_angle(big, 10 + r, 12 + r, r) - got) == 0
    img = np.zeros((21, 21), dtype=bool)
    img[10, 3:18] = True
    assert sk.direction(sk.window_sums(img, 10, 10, 6)) == (1.0, 0.0)            # horizontal
    assert sk.direction(sk.window_sums(img.T, 10, 10, 6)) == (0.0, 1.0)          # vertical: theta = pi / 2
    diag = np.eye(21, dtype=bool)
    h = np.sqrt(np.float64(0.5))
    assert sk.direction(sk.window_sums(diag, 10, 10, 6)) == (h, h)               # x and y grow together: 45 degrees
    assert sk.direction(sk.window_sums(diag[::-1], 10, 10, 6)) == (h, -h)
    assert sk.direction(sk.window_sums(diag, 0, 0, 6))[0] == h                   # a window that leaves the image
    assert sk.direction((1, 3, 4, 9, 12, 16)) == (1.0, 0.0) and sk.direction((0,) * 6) == (1.0, 0.0)


def test_locate_reference_and_its_stream():
    assert rng.LOCATE_STREAM == int.from_bytes(b"SKELLOC1", "big") and rng.STREAMS["locate"] == (rng.LOCATE_STREAM,)
    assert len({v for v in rng.STREAMS.values()}) == len(rng.STREAMS) and rng.MAX_DRAWS == 8
    keys = {name: rng.key(3, 1, name) for name in rng.STREAMS}
    assert len(set(keys.values())) == len(keys)
    for n in (1, 2, 57, 2 ** 18):
        draws = [rng.locate_reference(3, 1, n, row, k) for row in range(40) for k in range(8)]
        assert min(draws) >= 0 and max(draws) < n
        if n > 50:
            assert len(set(draws)) > 20
    h = rng.hi24(rng.hashes(rng.key(3, 1, "locate"), 16, 5 * 8))
    assert [rng.locate_reference(3, 1, 1000, 5, k) for k in range(8)] == [(int(v) * 1000) >> 24 for v in h[:8]]
    assert rng.locate_reference(3, 1, 1000, 5, 2) != rng.locate_reference(3, 2, 1000, 5, 2)
    with pytest.raises(ValueError):
        rng.locate_reference(0, 0, 10, 0, 8)


def test_each_draw_is_independent_of_num():
    m = _Morph(lc.skeletons()["blobs0"])
    sampler = sk.LocationSampler()
    eight = sampler.sample(m, 8, seed=2, counter=3, row=4)
    assert eight.shape == (8, 2) and m.skeleton[eight[:, 0], eight[:, 1]].all()
    for num in (1, 3, 5):
        assert np.array_equal(sampler.sample(m, num, 2, 3, 4), eight[:num])
    assert tuple(sampler.sample(m, None, 2, 3, 4)) == tuple(eight[0])
    coords = np.argwhere(m.skeleton)
    assert tuple(coords[rng.locate_reference(2, 3, len(coords), 4, 6)]) == tuple(eight[6])   # row-major
    assert not np.array_equal(sampler.sample(m, 8, 2, 3, 5), eight)


def test_line():
    ties = []
    g = np.random.default_rng(0)
    ends = [((0, 0), (0, 0)), ((3, 4), (3, 9)), ((3, 4), (9, 4)), ((0, 0), (5, 5)), ((2, 7), (-4, 1)), ((0, 0), (2, 4)),
            ((0, 0), (4, 2)), ((0, 0), (-1, 2)), ((5, 5), (4, -7))]
    ends += [(tuple(g.integers(-20, 20, 2)), tuple(g.integers(-20, 20, 2))) for _ in range(200)]
    for p0, p1 in ends:
        px = p.line(p0, p1)
        m = max(abs(p1[0] - p0[0]), abs(p1[1] - p0[1]))
        assert px.shape == (m + 1, 2) and tuple(px[0]) == tuple(p0) and tuple(px[-1]) == tuple(p1)
        step = np.diff(px, axis=0)
        assert (np.abs(step) <= 1).all() and (np.abs(step).max(1) == 1).all() if m else True     # 8-connected
        for axis in range(2):
            assert (step[:, axis] >= 0).all() or (step[:, axis] <= 0).all()                     # monotone
        back = p.line(p1, p0)[::-1]
        if not np.array_equal(px, back):
            # a reversed line differs only where the ideal line passes half way between two pixels: 2 t |dminor| is an
            # odd multiple of m there, and the rounding goes up from either end
            minor = 1 if abs(p1[0] - p0[0]) > abs(p1[1] - p0[1]) else 0
            dmin = abs(p1[minor] - p0[minor])
            where = np.nonzero((px != back).any(1))[0]
            assert all((2 * t * dmin) % (2 * m) == m for t in where), (p0, p1)
            ties.append((p0, p1))
    assert ((0, 0), (2, 4)) in ties and ((0, 0), (-1, 2)) in ties and ((0, 0), (5, 5)) not in ties


def _bar_morph(scale=4):
    image = mc.bar(3)
    morph = ImageMorphology(image, scale=scale)
    return image, morph


def test_swelling():
    _, morph = _bar_morph()
    binary = morph.binary_image
    centre = (56, 56)
    assert np.array_equal(p.Swelling(1)(morph, centre=centre), binary)           # strength 1: the identity
    R = p.swelling_radius(morph.mean_thickness, 7, morph.scale)
    out = p.Swelling(3, 7)(morph, centre=centre)
    y, x = np.mgrid[:112, :112]
    beyond = (y - 56) ** 2 + (x - 56) ** 2 > R * R
    assert beyond.any() and not beyond.all() and np.array_equal(out[beyond], binary[beyond])
    assert out[56, 56] == binary[56, 56] and out[56, 56]                         # the centre reads itself
    assert out.sum() > binary.sum() and out.dtype == bool                        # a bar swells
    drawn = p.Swelling()(morph, seed=1, counter=2, row=3)
    assert np.array_equal(drawn, p.Swelling()(morph, centre=sk.LocationSampler().sample(morph, None, 1, 2, 3)))
    odd = p.swell(binary, centre, R, 2.5)[0]                                     # through pow
    assert odd.sum() > binary.sum() and np.array_equal(odd[beyond], binary[beyond])
    with pytest.raises(ValueError, match="strength"):
        p.Swelling(0.5)


def test_fracture_on_a_horizontal_bar():
    H, W, width = 40, 80, 7
    binary = np.zeros((H, W), dtype=bool)
    binary[20 - width // 2:20 + width // 2 + 1, 5:75] = True
    skel = np.zeros_like(binary)
    skel[20, 8:72] = True
    d2 = np.rint(ndimage.distance_transform_edt(binary) ** 2).astype(np.int64)
    morph = _Morph(skel, scale=2, binary=binary, d2=d2)
    frac = p.Fracture(thickness=3, prune=2, num_frac=1)
    r = p.fracture_radius(3, 2)
    assert r == 3 and p.fracture_radius(0.1, 2) == 0 and p.fracture_radius(1.5, 16) == 12
    ends = p.fracture_endpoints(skel, d2, (20, 40), 2)
    assert ends == (20 + 5, 40, 20 - 5, 40)                          # L = sqrt(16) + 1, straight across the bar
    out = frac(morph, centres=[(20, 40)])
    cols = np.abs(np.arange(W) - 40) <= r
    want = binary.copy()
    want[:, cols] = False                                            # the line overshoots the bar by L - 3 > 0 rows
    assert np.array_equal(out, want)
    cells = lambda im: [tuple(c) for c in np.argwhere(im)]
    assert _components(cells(out)) == _components(cells(binary)) + 1
    # a cut next to the border keeps the part of its stamps that lies inside the image
    edge = np.zeros((12, 30), dtype=bool)
    edge[0:4, :] = True
    eskel = np.zeros_like(edge)
    eskel[1, 2:28] = True
    ed2 = np.rint(ndimage.distance_transform_edt(edge) ** 2).astype(np.int64)
    em = _Morph(eskel, scale=2, binary=edge, d2=ed2)
    ends = p.fracture_endpoints(eskel, ed2, (1, 15), 2)
    assert ends[2] < 0                                               # the line leaves the image at the top
    cut = frac(em, centres=[(1, 15)])
    want = edge.copy()
    want[:, np.abs(np.arange(30) - 15) <= r] = False
    assert np.array_equal(cut, want)
    drawn = p.Fracture(3, 2, 3).centres(morph, seed=4)
    assert drawn[0].shape == (3, 2) and drawn[2] == 0 and drawn[1] == int(sk.candidates(skel, 2, 2, 2).sum())
    over = p.Fracture(3, 40, 3).centres(morph, seed=4)
    assert over[2] == 1 and over[1] == int(skel.sum())               # overpruned: the same draws of the whole skeleton
    assert np.array_equal(over[0], sk.LocationSampler().sample(morph, 3, 4))
    for bad in (0, 9):
        with pytest.raises(ValueError, match="num_frac"):
            p.Fracture(num_frac=bad)


def test_small_images_overprune_and_strokes_do_not():
    """what the GPU tests rely on: pruning leaves 0 .. 2 pixels of the 5 x 9 images' skeletons, so some fall back to the
    whole skeleton; the 28 x 28 strokes keep most of theirs"""
    fell = 0
    for H, W, s in mc.SMALL:
        for b, image in enumerate(mc.image_batch(3, H, W)):
            out = p.local_image(image, "fracture", scale=s)
            pruned = int(sk.LocationSampler(2, 2).candidates(ImageMorphology(image, scale=s)).sum())
            assert out["status"] in (0, 4) and out["n_candidates"] > 0, (H, W, s, b)     # (4: a cut may leave nothing)
            assert out["fallback"] == (pruned == 0) and (pruned <= 2 if H == 5 else pruned >= 40), (H, W, s, b, pruned)
            fell += out["fallback"]
    assert fell >= 3


def test_local_image_status_and_kinds():
    image = mc.image_batch(1, 28, 28)[0]
    plain = p.local_image(image, "plain", scale=4)
    morph = ImageMorphology(image, scale=4)
    assert plain["status"] == 0 and np.array_equal(plain["bitmap"], morph.binary_image)
    assert np.array_equal(plain["image"], morph.downscale(morph.binary_image))
    thin = p.local_image(image, 1, scale=4)
    assert np.array_equal(thin["bitmap"], p.Thinning()(morph)) and thin["radius"] == int(.7 * 4 * morph.mean_thickness / 2)
    thick = p.local_image(image, "thick", scale=4)
    assert np.array_equal(thick["bitmap"], p.Thickening()(morph))
    assert p.local_image(image, "thin", scale=4, thin_amount=3.)["status"] == 4  # thinned away
    assert p.local_image(np.full((28, 28), .3), "swell", scale=4)["status"] == 1
    assert p.local_image(image, 7, scale=4)["status"] == 4
    with pytest.raises(ValueError, match="kind"):
        p.local_image(image, "swollen", scale=4)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_morpho_local_on_cpu_tensors_is_the_row_loop(dtype):
    x = torch.from_numpy(mc.generator_images(3, seed=2)).to(dtype)
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    ml = MorphoLocal(scale=4, seed=5)
    mixed = torch.tensor([4, 3, 1], dtype=torch.int32)
    for call, kind in enumerate(lc.KINDS + (mixed,)):
        out = ml.apply(x, kind)
        assert out["images"].dtype == dtype and out["images"].shape == (3, 28, 28)
        maps = unpack_bits(out["bits"], 112)
        for b in range(3):
            k = kind if isinstance(kind, str) else int(kind[b])
            want = p.local_image(x[b].numpy(), k, 4, .5, 5, np_dtype, counter=call, row=b)
            assert np.array_equal(maps[b], want["bitmap"]) and np.array_equal(out["images"][b].numpy(), want["image"])
            for key in lc.INT_KEYS:
                assert int(out[key][b]) == want[key], (kind, b, key)
            assert np.array_equal(out["centres"][b].numpy(), want["centres"])
            assert np.array_equal(out["endpoints"][b].numpy(), want["endpoints"])
    assert ml.calls == 6


def test_refusals():
    x = torch.zeros(2, 28, 28)
    ml = MorphoLocal(scale=4)
    with pytest.raises(ValueError, match="kind"):
        ml.apply(x, "swollen")
    with pytest.raises(ValueError, match="kind"):
        ml.apply(x, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="kind"):
        ml.apply(x, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="num_frac"):
        MorphoLocal(num_frac=9)
    with pytest.raises(ValueError, match="swell_strength"):
        MorphoLocal(swell_strength=0.5)
    with pytest.raises(ValueError, match="exceed the limit"):
        MorphoLocal(scale=16).apply(torch.zeros(1, 33, 28), "plain")
