"""Shared by tests/test_morphomnist_cpu.py, tests/test_gpu_morpho_kernels.py and tests/test_gpu_morphomnist.py: the
synthetic images, binary images and skeletons of the morphomnist family's tests, and the statement of the scripts'
``extract_observed_attributes`` written out."""
import numpy as np

SMALL = [(5, 9, 1), (5, 9, 2), (5, 9, 4), (28, 28, 4)]          # (H, W, scale); 28 x 28 at scale 16 runs with B = 3
BATCHES = (1, 3, 70)


def bar(w, H=28, W=28, length=16):
    """a vertical bar of width w and the given length, 0 / 1"""
    im = np.zeros((H, W))
    y0, x0 = (H - length) // 2, (W - w) // 2
    im[y0:y0 + length, x0:x0 + w] = 1
    return im


def ring(radius=7, w=3, H=28, W=28):
    y, x = np.mgrid[:H, :W]
    d = np.hypot(y - (H - 1) / 2, x - (W - 1) / 2)
    return ((d >= radius - w / 2) & (d <= radius + w / 2)).astype(float)


def stroke(H=28, W=28, seed=0, amplitude=1.0, noise=0.0):
    """A smooth pen stroke: a quadratic curve from the upper to the lower third of the image, drawn with a Gaussian
    profile (peak ``amplitude``, background 0, width at half height 2.1 .. 3.1 pixels at 28 x 28), plus Gaussian noise
    of standard deviation ``noise`` in units where the peak is 255.  At 28 x 28 it is some 20 pixels long: 600 .. 950
    foreground pixels at scale 4 and 10 .. 15 thousand at scale 16, the size of a handwritten digit's stroke."""
    g = np.random.default_rng(1000 + seed)
    t = np.linspace(0, 1, 200)
    lo, hi = np.array([0.15, 0.15]), np.array([0.35, 0.85])
    p = np.stack([g.uniform(lo, hi), g.uniform(0.2, 0.8, size=2), g.uniform(1 - hi, 1 - lo)]) * [H - 1, W - 1]
    curve = ((1 - t) ** 2)[:, None] * p[0] + (2 * t * (1 - t))[:, None] * p[1] + (t ** 2)[:, None] * p[2]
    y, x = np.mgrid[:H, :W]
    d2 = ((y[..., None] - curve[:, 0]) ** 2 + (x[..., None] - curve[:, 1]) ** 2).min(-1)
    sigma = max(g.uniform(0.9, 1.3) * min(H, W) / 28, 0.6)
    im = amplitude * np.exp(-d2 / (2 * sigma ** 2))
    if noise:
        im = im + amplitude * noise / 255 * g.standard_normal(im.shape)
    return im


def image_batch(B, H, W, seed=0):
    """[B, H, W] float64 in 0 .. 1: strokes, every fourth with noise of sigma 4 / 255; at 28 x 28 the second and third
    are the bar of width 3 and the ring"""
    ims = [stroke(H, W, seed * 131 + b, noise=4.0 if b % 4 == 3 else 0.0) for b in range(B)]
    if (H, W) == (28, 28) and B >= 3:
        ims[1], ims[2] = bar(3), ring()
    return np.stack(ims)


def generator_images(B, H=28, W=28, seed=0):
    """[B, H, W] float32 in -1 .. 1, as a Generator's tanh writes them: ``2 * image_batch - 1`` rounded to fp32 and
    clipped, so that the far background is -1 exactly (the scripts' ``255 * (x + 1) / 2`` then has a background of 0)"""
    x = np.clip(2 * image_batch(B, H, W, seed) - 1, -1, 1).astype(np.float32)
    assert (x.reshape(B, -1).min(1) == -1).all()
    return x


def blobs(H, W, seed=0, fill=0.45):
    """a random binary image with large plateaus: a smoothed random field above its ``1 - fill`` quantile"""
    from scipy import ndimage
    g = np.random.default_rng(77 + seed)
    f = ndimage.gaussian_filter(g.standard_normal((H, W)), max(min(H, W) / 12, 1.0), mode="wrap")
    return f >= np.quantile(f, 1 - fill)


def binary_cases(H, W, seed=0):
    """{name: bool [H, W]}: the built binary images of the distance-map and thinning tests"""
    full = np.ones((H, W), dtype=bool)
    hole = full.copy()
    hole[H // 3, (2 * W) // 3] = False
    frame = np.zeros((H, W), dtype=bool)                         # foreground on all four borders, background inside
    frame[[0, -1], :] = True
    frame[:, [0, -1]] = True
    frame[: max(H // 4, 1), : max(W // 4, 1)] = True
    rows = np.zeros((H, W), dtype=bool)                          # full rows (no background in them) and full columns
    rows[1::3, :] = True
    rows[:, W // 2] = True
    lines = np.zeros((H, W), dtype=bool)                         # one-pixel lines: horizontal, vertical, diagonal
    lines[H // 2, 1:W - 1] = True
    lines[1:H - 1, W // 3] = True
    n = min(H, W)
    lines[np.arange(n), np.arange(n)] = True
    bars = np.zeros((H, W), dtype=bool)                          # two-wide bars, one touching the border
    bars[1:H - 1, 1:3] = True
    bars[H - 2:, :] = True
    bars[0:2, W // 2:] = True
    one = np.zeros((H, W), dtype=bool)
    one[H // 2, W // 2] = True
    return {"blobs": blobs(H, W, seed), "blobs2": blobs(H, W, seed + 1, 0.7), "hole": hole, "frame": frame,
            "rows": rows, "lines": lines, "bars": bars, "one": one, "empty": np.zeros((H, W), dtype=bool)}


def skeleton_cases(H=7, W=40):
    """{name: (bool [H, W], straight pairs, diagonal pairs)}: hand-built skeletons with their pair counts"""
    def blank():
        return np.zeros((H, W), dtype=bool)
    run = blank()
    run[3, 2:W - 1] = True                                       # crosses the word boundary at x = 32
    col = blank()
    col[1:H, W - 1] = True
    diag = blank()
    diag[np.arange(H), 29 + np.arange(H)] = True                 # crosses x = 32 going down-right
    anti = blank()
    anti[np.arange(H), 34 - np.arange(H)] = True                 # crosses x = 32 going down-left
    ell = blank()
    ell[1:5, 31] = True
    ell[4, 31:36] = True
    block = blank()
    block[2:4, 31:33] = True                                     # 2 x 2 on the word boundary
    return {"run": (run, W - 4, 0), "col": (col, H - 2, 0), "diag": (diag, 0, H - 1), "anti": (anti, 0, H - 1),
            "ell": (ell, 3 + 4, 1), "block": (block, 4, 2), "none": (blank(), 0, 0)}


def extract_observed_attributes(image, scale=16):
    """The function of mnist_gan_measured_cf.py / mnist_vae_measured_cf.py, on any image shape: (thickness, intensity,
    slant) of one image through ``morphomnist.morpho``"""
    from morphomnist.morpho import ImageMoments, ImageMorphology
    morph = ImageMorphology(image, scale=scale)
    thickness = morph.mean_thickness
    img_min, img_max = image.min(), image.max()
    intensity = np.median(image[image >= img_min + (img_max - img_min) * .5])
    moments = ImageMoments(image)
    slant = -moments.horizontal_shear
    return np.array([thickness, intensity, slant])
