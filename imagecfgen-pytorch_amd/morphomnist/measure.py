"""``morphomnist.measure`` of the reference package: ``Morphometrics``, ``measure_image`` and ``measure_batch``.

``measure_image`` measures the statement of ``morphomnist.morpho``: area, length and thickness of ``ImageMorphology``
(seed 0), and slant, width and height of ``measure_bounds`` -- the moments and the bounding parallelogram of hires =
expand(image - image.min(), scale), the crossings of the non-monotone cdfs by ``quantile_loc``.
``measure_batch`` runs it row by row (or through ``pool.imap``) for numpy and CPU input; a CUDA tensor goes through
``ali_hip.morpho.MorphoMeasure(bound_frac=...)`` on the device, with a single host read.
"""
import multiprocessing
from typing import NamedTuple

import numpy as np
import pandas as pd

from .morpho import ImageMorphology, measure_bounds

FIELDS = ("area", "length", "thickness", "slant", "width", "height")


class Morphometrics(NamedTuple):
    """Measured shape attributes of an image: area (image mass), length (of the skeleton), thickness (mean, along the
    skeleton), slant (horizontal shear, in radians), width and height (of the bounding parallelogram)."""
    area: float
    length: float
    thickness: float
    slant: float
    width: float
    height: float


def measure_image(image, threshold: float = .5, scale: int = 4, bound_frac: float = .02, verbose=True):
    """The morphometrics of one image [H, W] (see the module's docstring); ``verbose`` prints them."""
    image = np.asarray(image)
    morph = ImageMorphology(image, threshold, scale, seed=0)
    thickness = morph.mean_thickness
    area = morph.area
    length = morph.stroke_length
    b = measure_bounds(image, scale, bound_frac)
    slant, width, height = b["slant"], b["width"], b["height"]

    if verbose:
        print(f"Area: {area:.1f}")
        print(f"Length: {length:.1f}")
        print(f"Thickness: {thickness:.2f}")
        print(f"Slant: {np.rad2deg(slant):.0f}°")
        print(f"Dimensions: {width:.1f} x {height:.1f}")

    return Morphometrics(area, length, thickness, slant, width, height)


def _measure_image_unpack(arg):
    return measure_image(*arg)


def _progress(gen, n):
    try:
        import tqdm
        return tqdm.tqdm(gen, total=n, unit='img', ascii=True)
    except ImportError:
        def plain_progress(g):
            print(f"\rProcessing images: {0}/{n}", end='')
            for i, res in enumerate(g):
                print(f"\rProcessing images: {i + 1}/{n}", end='')
                yield res
            print()
        return plain_progress(gen)


def measure_batch(images, threshold: float = .5, scale: int = 4, bound_frac: float = .02,
                  pool: multiprocessing.Pool = None, chunksize: int = 100) -> pd.DataFrame:
    """A DataFrame with one row of ``Morphometrics`` per image of ``images`` [N, H, W] (numpy, a CPU tensor, or a CUDA
    tensor: see the module's docstring; ``pool`` and ``chunksize`` apply to the host path)."""
    import torch
    if torch.is_tensor(images) and images.is_cuda:
        from ali_hip.morpho import MorphoMeasure
        mm = MorphoMeasure(scale=scale, threshold=threshold, seed=0, bound_frac=bound_frac)
        mm.measure(images)
        tab = mm.table()                                             # the one host read
        return pd.DataFrame({"area": tab["area"], "length": tab["length"], "thickness": tab["thickness"],
                             "slant": tab["slant_measure"], "width": tab["width"], "height": tab["height"]},
                            columns=list(FIELDS))
    if torch.is_tensor(images):
        images = images.detach().numpy()
    images = np.asarray(images)
    args = ((img, threshold, scale, bound_frac, False) for img in images)
    if pool is None:
        gen = map(_measure_image_unpack, args)
    else:
        gen = pool.imap(_measure_image_unpack, args, chunksize=chunksize)
    results = list(_progress(gen, len(images)))
    return pd.DataFrame(results, columns=list(FIELDS))
