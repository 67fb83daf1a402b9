"""Shared by tests/test_morphomnist_perturb_cpu.py, tests/test_gpu_morpho_perturb_kernels.py and
tests/test_gpu_morphomnist_perturb.py: built bitmaps, thickness / target pairs that hit chosen radii, half-width tables
with only the rows a test needs, and the scripts' loop body written out on the statement."""
import numpy as np

import morpho_cases as mc

RADII = (1, 2, 3, 5, 8, 13, 24, 40)
SET_PIXELS = (9, 25, 49, 121, 277, 669, 2081, 5501)              # of footprint(r), scipy 1.15.3
DISK_PIXELS = (5, 13, 29, 81, 197, 529, 1793, 5025)              # of the exact disk(r)


def built(Hh, Wh, B):
    """B built binary images [B, Hh, Wh]: the cases of ``morpho_cases.binary_cases`` in turn (blobs, a hole, a frame and
    bars on the border, one-pixel lines, one pixel, the empty image), with another seed each time round"""
    out = []
    while len(out) < B:
        out += list(mc.binary_cases(Hh, Wh, seed=len(out)).values())
    return np.stack(out[:B])


def radius_targets(B, scale, max_radius, thickness=3.0):
    """(thickness, target, radius): fp32 [B], fp32 [B], int [B].  Row b asks for the signed radius
    (0, 1, -1, 2, -2, 5, -5, max, -max, max + 1, -(max + 3))[b % 11]: target = thickness + 2 * (r +- 0.5) / scale, half a
    pixel inside the radius, so the rounding of the two fp32 values (1e-7) cannot move it."""
    want = np.array([(0, 1, -1, 2, -2, 5, -5, max_radius, -max_radius, max_radius + 1, -(max_radius + 3))[b % 11]
                     for b in range(B)])
    sign = np.where(want < 0, -1.0, 1.0)
    thick = np.full(B, thickness, dtype=np.float32)
    target = (thick.astype(np.float64) + sign * 2 * (np.abs(want) + 0.5) / scale).astype(np.float32)
    return thick, target, want


def sparse_table(max_radius, radii):
    """``perturb.half_width_table(max_radius)`` with only the rows of ``radii`` filled in (the others are never read by a
    test that asks for those radii alone; building all of 0 .. 64 takes seconds)"""
    from morphomnist import perturb
    table = np.full((max_radius + 1, 2 * max_radius + 1), -1, dtype=np.int16)
    for r in radii:
        table[r, :2 * r + 1] = perturb.half_widths(r)
    return table


def script_loop_body(im, th, sl, in_, scale):
    """mnist_vae_measured_cf.py:68-74 for one image, on the statement"""
    from morphomnist.morpho import ImageMorphology
    from morphomnist.perturb import SetSlant, SetThickness
    morph = ImageMorphology(im, scale=scale)
    new_img = np.float32(SetThickness(th)(morph))
    new_img = morph.downscale(np.float32(SetSlant(sl)(ImageMorphology(new_img))))
    img_min, img_max = new_img.min(), new_img.max()
    current_intensity = np.median(new_img[new_img >= img_min + (img_max - img_min) * .5])
    mult = in_ / current_intensity
    return np.clip(new_img * mult, 0, 255)


def sheared_bar(k, Hh=96, Wh=96, w=9, length=64):
    """(bitmap, x0, rows): a vertical bar of width w whose row y is moved by round(k * (y - cy)) columns"""
    y0, x0 = (Hh - length) // 2, (Wh - w) // 2
    rows = np.arange(y0, y0 + length)
    cy = rows.mean()
    out = np.zeros((Hh, Wh), dtype=bool)
    for y in rows:
        sh = int(np.floor(0.5 + k * (y - cy)))
        out[y, x0 + sh:x0 + sh + w] = True
    return out, x0, rows
