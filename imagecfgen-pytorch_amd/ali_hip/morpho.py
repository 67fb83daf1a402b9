"""Executor of the morphomnist family: the measurement loop of ``mnist_gan_measured_cf.py`` and
``mnist_vae_measured_cf.py`` -- ``extract_observed_attributes`` for every generated image -- as one call per batch.

  MorphoMeasure   ``measure(images)`` returns thickness, intensity and slant (the scripts' three columns) plus area,
                  stroke length, the slant of the up-sampled image, the counts behind them and a status per image, as
                  device tensors with no host read: four launches per chunk (csrc/morpho.hip: binarise, distance map,
                  thinning, measures).  ``table()`` is the one host read.
  MorphoPerturb   ``apply(images, thickness, slant, intensity)`` returns the ground-truth counterfactual images of
                  ``mnist_vae_measured_cf.py`` and the data-set builders -- ``SetThickness``, ``SetSlant``, ``downscale``,
                  the intensity rescale -- as device tensors with no host read: the four launches above and three more
                  per chunk (reshape, shear_reduce, set_intensity).  ``set_width(images, width, intensity)`` is
                  ``SetWidth`` and ``downscale``: binarise, width, affine_reduce per chunk, and the reference's
                  validation as one re-application selected per row on the device.
  MorphoLocal     ``apply(images, kind)`` returns the images of the five Morpho-MNIST data sets -- plain, ``Thinning``,
                  ``Thickening``, ``Swelling``, ``Fracture`` and ``downscale`` -- as device tensors with no host read: the four
                  launches above, then locate, local and shear_reduce (and one more distance map for "thick").

CPU tensors run the statement ``morphomnist.morpho`` row by row in the dtype of the tensor (float64: the tests'
reference; float32: their yardstick), and ``morphomnist.perturb`` likewise.  What is measured and perturbed is that
statement, not scikit-image's pipeline.
"""
import numpy as np
import torch

from morphomnist import morpho as stmt

from . import ops

COLUMNS = ("thickness", "intensity", "slant", "area", "length", "slant_hires")
BOUND_COLUMNS = ("width", "height", "slant_measure")             # with MorphoMeasure(bound_frac=...)
WORKSPACE_BUDGET = 384 << 20     # bytes of scratch, distance maps and bitmaps one chunk may hold


def pack_bits(images):
    """boolean images [B, Hh, Wh] (numpy) -> the bitmap words int32 [B, Hh, ceil(Wh / 32)] (a CPU tensor)"""
    images = np.asarray(images, dtype=bool)
    B, Hh, Wh = images.shape
    wpr = (Wh + 31) // 32
    padded = np.zeros((B, Hh, wpr * 32), dtype=bool)
    padded[:, :, :Wh] = images
    return torch.from_numpy(np.packbits(padded, axis=2, bitorder="little").view(np.int32).reshape(B, Hh, wpr).copy())


def unpack_bits(words, Wh):
    """bitmap words [B, Hh, wpr] (a tensor on any device) -> boolean images [B, Hh, Wh] (numpy)"""
    w = words.detach().cpu().numpy().view(np.uint8)
    return np.unpackbits(w, axis=2, bitorder="little")[:, :, :Wh].astype(bool)


def scratch_bytes(H, W, scale, bounds=False):
    """the largest scratch per image of the three kernels that use one (binarise, edt, thin), and of bounds when it
    runs"""
    need = max(4 * H * W * scale if scale > 1 else 0, 2 * H * W * scale * scale)
    return max(need, ops.morpho_bounds_scratch_bytes(H, W, scale)) if bounds else need


def per_image_bytes(H, W, scale, bounds=False):
    """what one image of a chunk holds on the device: scratch, the distance map and the two bitmaps"""
    Hh, Wh = H * scale, W * scale
    return scratch_bytes(H, W, scale, bounds) + 4 * Hh * Wh + 2 * 4 * Hh * ((Wh + 31) // 32)


def as_images(images):
    """[B, 1, H, W], [B, H, W] or [B, H * W] (square) -> [B, H, W]"""
    if images.dim() == 4 and images.shape[1] == 1:
        return images[:, 0]
    if images.dim() == 3:
        return images
    if images.dim() == 2:
        n = int(round(images.shape[1] ** 0.5))
        if n * n == images.shape[1]:
            return images.reshape(images.shape[0], n, n)
    raise ValueError(f"MorphoMeasure: need [B, 1, H, W], [B, H, W] or square [B, H * W] images, got "
                     f"{tuple(images.shape)}")


def checked_images(images, who, scale):
    """``as_images`` of float images within the up-sampling limit -> (x [B, H, W], B, H, W); on a GPU x is fp32 with
    contiguous images, what the launches take"""
    x = as_images(images)
    if not x.is_floating_point():
        raise ValueError(f"{who}: float images only")
    B, H, W = x.shape
    if H * scale > ops.MORPHO_MAX_SIDE or W * scale > ops.MORPHO_MAX_SIDE:
        raise ValueError(f"{who}: {H} x {W} images at scale {scale} exceed the limit of "
                         f"{ops.MORPHO_MAX_SIDE} x {ops.MORPHO_MAX_SIDE} up-sampled pixels")
    if x.is_cuda and (x.dtype != torch.float32 or not x[0].is_contiguous()):
        x = x.float().contiguous()
    return x, B, H, W


def statement_row(image, scale=16, threshold=.5, seed=0, dtype=np.float64, binary=None):
    """One image through the statement: (counts [4] int64, values [5], slant_hires, status), the floats in ``dtype``.
    ``binary``: continue from this binary image instead of the statement's own."""
    image = np.asarray(image, dtype=dtype)
    m = stmt.ImageMorphology(image, threshold, scale, seed, dtype, binary=binary)
    straight, diagonal = stmt.skeleton_pairs(m.skeleton)
    counts = np.array([m.binary_image.sum(), m.skeleton.sum(), straight, diagonal], dtype=np.int64)
    values = np.array([m.area, m.stroke_length, m.mean_thickness, stmt.intensity(image),
                       -stmt.ImageMoments(image - image.min(), dtype).horizontal_shear], dtype=dtype)
    slant_hires = np.arctan(-stmt.ImageMoments(m.hires_image - m.hires_image.min(), dtype).horizontal_shear)
    return counts, values, dtype(slant_hires), m.status


class MorphoMeasure:
    """``extract_observed_attributes`` of the measured-counterfactual scripts for a batch.

    ``measure(images)`` takes [B, 1, H, W], [B, H, W] or [B, H * W] (square) float tensors, in the Generator's range
    (-1 .. 1) or in 0 .. 255.  Every measure but ``intensity`` is unchanged by a positive affine map of the pixel
    values: the threshold is relative, and the moments behind the two slants are those of the image less its minimum
    -- for the scripts' ``255 * (x + 1) / 2`` with a background of 0 exactly the moments ``ImageMoments(image)`` takes.
    ``intensity`` is returned in the units of the input.

    Returns {"thickness", "intensity", "slant" (the scripts' -u11 / u02), "area", "length", "slant_hires"
    (atan of the same ratio on the up-sampled image): float32 [B]; "counts": int32 [B, 4] = foreground, skeleton,
    straight pairs, diagonal pairs; "status": int32 [B], 0, or 1 for an image without background (NaN thickness, area,
    length), or 2 if the thinning did not finish}.  Limit: H * scale and W * scale up to 512.

    CUDA tensors: four launches per chunk of ``chunk`` images, no host read; the default chunk is what fits
    ``WORKSPACE_BUDGET`` (306 images of 28 x 28 at scale 16, 1.25 MB each), so memory is bounded whatever B is.
    ``table()`` returns every row measured so far as numpy columns with one host read; ``reset()`` forgets them.

    ``bound_frac`` (0 < bound_frac < 1, or None): the bounding parallelogram of ``morphomnist.measure.measure_image``
    too, on hires = expand(image - image.min()) -- one more launch per chunk (csrc/morpho.hip: bounds), still no host
    read.  It adds "width", "height" ((right - left) / scale, (bottom - top) / scale) and "slant_measure" (atan(-u11 /
    u02) of hires): float32 [B]; "bounds": float64 [B, 6] = left, right, top, bottom, shear, middle in up-sampled pixels;
    "corners": float64 [B, 4, 2], (x, y) clockwise from the top left; NaN without mass or with a shear that is not
    finite.  None: every output, the chunk and the launches are those above."""

    def __init__(self, scale=16, threshold=.5, seed=0, chunk=None, bound_frac=None):
        self.scale, self.threshold, self.seed = int(scale), float(threshold), int(seed)
        if self.scale < 1:
            raise ValueError("MorphoMeasure: scale >= 1")
        if bound_frac is not None and not 0.0 < float(bound_frac) < 1.0:
            raise ValueError(f"MorphoMeasure: 0 < bound_frac < 1, or None; got {bound_frac}")
        self.bound_frac = None if bound_frac is None else float(bound_frac)
        self.chunk = chunk
        self._ops, self._ws, self._blocks = {}, {}, []
        self._keep = stmt.keep_bits()

    def chunk_for(self, H, W):
        if self.chunk is not None:
            return max(int(self.chunk), 1)
        return max(WORKSPACE_BUDGET // per_image_bytes(H, W, self.scale, self.bound_frac is not None), 1)

    def operators(self, H, W, device):
        """(AH, AW): the expand operators as fp32 device tensors, built once per size in fp64 on the host"""
        key = (H, W, str(device))
        if key not in self._ops:
            self._ops[key] = tuple(torch.from_numpy(stmt.expand_operator(n, self.scale).astype(np.float32)).to(device)
                                   for n in (H, W)) if self.scale > 1 else (None, None)
        return self._ops[key]

    def _workspace(self, n, H, W, device):
        need = ops.WS_RESERVED + n * scratch_bytes(H, W, self.scale, self.bound_frac is not None)
        ws = self._ws.get(str(device))
        if ws is None or ws.numel() < need:
            ws = self._ws[str(device)] = torch.zeros(need, dtype=torch.uint8, device=device)
        return ws

    def _bounds_columns(self, bounds, dtype):
        """width, height, slant_measure in ``dtype`` and the corners [B, 4, 2] from bounds [B, 6] (float64, any
        device), each operation on its own as the statement takes them"""
        left, right, top, bottom, shear, middle = bounds.unbind(1)
        s = float(self.scale)
        width, height = ((right - left) / s).to(dtype), ((bottom - top) / s).to(dtype)
        slant = torch.atan(-shear).to(dtype)
        at_top, at_bottom = shear * (top - middle), shear * (bottom - middle)
        corners = torch.stack([torch.stack([left + at_top, top], 1), torch.stack([right + at_top, top], 1),
                               torch.stack([right + at_bottom, bottom], 1), torch.stack([left + at_bottom, bottom], 1)],
                              1)
        return width, height, slant, corners

    @torch.no_grad()
    def measure(self, images):
        x, B, H, W = checked_images(images, "MorphoMeasure", self.scale)
        if not x.is_cuda:
            return self._remember(*self._measure_cpu(x))
        dev = x.device
        counts = torch.empty(B, 4, dtype=torch.int32, device=dev)
        values = torch.empty(B, 5, dtype=torch.float32, device=dev)
        slant = torch.empty(B, dtype=torch.float32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        AH, AW = self.operators(H, W, dev)
        n = min(self.chunk_for(H, W), B)
        ws = self._workspace(n, H, W, dev)
        bounds = None if self.bound_frac is None else torch.empty(B, 6, dtype=torch.float64, device=dev)
        for lo in range(0, B, n):
            hi = min(lo + n, B)
            bits, fg, hstats = ops.morpho_binarise(x[lo:hi], self.scale, AH, AW, self.threshold, ws=ws)
            d2, st = ops.morpho_edt(bits, W * self.scale, ws=ws)
            skel = ops.morpho_thin(bits, d2, fg, st, self._keep, self.seed, ws=ws)
            ops.morpho_measure(x[lo:hi], self.scale, skel, d2, fg, hstats, st,
                               out=(counts[lo:hi], values[lo:hi], slant[lo:hi]))
            status[lo:hi] = st
            if bounds is not None:
                ops.morpho_bounds(x[lo:hi], self.scale, AH, AW, self.bound_frac, ws=ws, out=bounds[lo:hi])
        extra = None if bounds is None else (*self._bounds_columns(bounds, torch.float32), bounds)
        return self._remember(counts, values, slant, status, extra)

    def _measure_cpu(self, x):
        dtype = np.float64 if x.dtype == torch.float64 else np.float32
        rows = [statement_row(img.numpy(), self.scale, self.threshold, self.seed, dtype) for img in x]
        extra = None
        if self.bound_frac is not None:
            got = [stmt.measure_bounds(img.numpy(), self.scale, self.bound_frac, dtype) for img in x]
            col = lambda k: torch.from_numpy(np.array([g[k] for g in got], dtype=dtype))
            extra = (col("width"), col("height"), col("slant"), torch.from_numpy(np.stack([g["corners"] for g in got])),
                     torch.from_numpy(np.stack([g["bounds"] for g in got])))
        return (torch.from_numpy(np.stack([r[0] for r in rows]).astype(np.int32)),
                torch.from_numpy(np.stack([r[1] for r in rows])),
                torch.from_numpy(np.array([r[2] for r in rows], dtype=dtype)),
                torch.tensor([r[3] for r in rows], dtype=torch.int32), extra)

    def _remember(self, counts, values, slant, status, extra=None):
        out = {"area": values[:, 0], "length": values[:, 1], "thickness": values[:, 2], "intensity": values[:, 3],
               "slant": values[:, 4], "slant_hires": slant, "counts": counts, "status": status}
        # one block of float64 per call: the integers are exact in it, and ``table`` reads every block at once
        block = [values.double(), slant.double().reshape(-1, 1), counts.double(), status.double().reshape(-1, 1)]
        if extra is not None:
            width, height, slant_measure, corners, bounds = extra
            out.update(width=width, height=height, slant_measure=slant_measure, bounds=bounds, corners=corners)
            block += [torch.stack([width, height, slant_measure], 1).double(), bounds, corners.reshape(-1, 8)]
        self._blocks.append(torch.cat(block, dim=1))
        return out

    def table(self):
        """{column: numpy array} of every row measured so far, in order (one host read): the float columns of
        ``COLUMNS``, ``counts`` int64 [N, 4] and ``status`` int64 [N]; with ``bound_frac`` also those of
        ``BOUND_COLUMNS``, ``bounds`` [N, 6] and ``corners`` [N, 4, 2]"""
        wide = self.bound_frac is not None
        if not self._blocks:
            host = np.zeros((0, 28 if wide else 11))
        else:
            host = torch.cat(self._blocks).cpu().numpy()
        out = {"area": host[:, 0], "length": host[:, 1], "thickness": host[:, 2], "intensity": host[:, 3],
               "slant": host[:, 4], "slant_hires": host[:, 5]}
        out["counts"] = host[:, 6:10].astype(np.int64)
        out["status"] = host[:, 10].astype(np.int64)
        if wide:
            out.update(width=host[:, 11], height=host[:, 12], slant_measure=host[:, 13], bounds=host[:, 14:20],
                       corners=host[:, 20:28].reshape(-1, 4, 2))
        return out

    def reset(self):
        self._blocks = []


def perturb_scratch_bytes(H, W, scale):
    """the largest scratch per image of the seven launches: the four of ``scratch_bytes``, reshape's row distances
    (uint16 per up-sampled pixel) and shear_reduce's T (float64 [H * scale, W])"""
    return max(scratch_bytes(H, W, scale), 2 * H * W * scale * scale, 8 * H * W * scale if scale > 1 else 0)


def perturb_image_bytes(H, W, scale):
    """what one image of a ``MorphoPerturb`` chunk holds on the device: ``per_image_bytes`` with the scratch of all seven
    launches, the reshaped bitmap, the quantised and the rescaled image and the moment sums"""
    Hh, Wh = H * scale, W * scale
    scratch = perturb_scratch_bytes(H, W, scale)
    return (per_image_bytes(H, W, scale) - scratch_bytes(H, W, scale) + scratch + 4 * Hh * ((Wh + 31) // 32)
            + 2 * 4 * H * W + 6 * 8)


def width_scratch_bytes(H, W, scale):
    """the largest scratch per image of the ``set_width`` chain: binarise's T (fp32 [H, W * scale]), width's T when it
    does not fit in LDS, affine_reduce's T (float64 [H * scale, W]), and bounds' for ``validate``"""
    return max(4 * H * W * scale, 8 * H * W * scale, ops.morpho_bounds_scratch_bytes(H, W, scale)) if scale > 1 else 0


def width_image_bytes(H, W, scale):
    """what one image of a ``MorphoPerturb.set_width`` chunk holds on the device: the scratch, the bitmap, two rounds
    of the quantised image with the selected and the rescaled one, and the sums, values and statuses"""
    Hh, Wh = H * scale, W * scale
    return width_scratch_bytes(H, W, scale) + 2 * 4 * Hh * ((Wh + 31) // 32) + 4 * 4 * H * W + 4 * (6 * 8 + 6 * 8 + 16)


class MorphoPerturb:
    """The ground-truth counterfactual image of ``mnist_vae_measured_cf.py`` / ``mnist_vae_counterfactuals.py`` and the
    data-set builders for a batch: ``SetThickness``, ``SetSlant``, ``downscale`` and the intensity rescale of
    ``morphomnist.perturb.counterfactual_image``.

    ``apply(images, thickness=None, slant=None, intensity=None)`` takes images as ``MorphoMeasure.measure`` does (-1 .. 1
    or 0 .. 255: the bitmap does not depend on it) and targets as [B] tensors on the images' device, or None (radius 0 /
    no shear / no rescale).  Returns {"images": float [B, H, W] in 0 .. 255, "status": int32 [B] (0; 1, 2 as
    ``MorphoMeasure``; 3: radius > max_radius; 4: nothing left to work with -- the image is 0 then), "radius": int32 [B]
    (signed: dilate >= 0 > erode), "thickness_before": the measured thickness, "shear_before": float64 [B], u11 / u02 of
    the reshaped bitmap, "intensity_before": the median of the quantised image}.

    CUDA tensors: per chunk the four launches of ``MorphoMeasure`` and three more (csrc/morpho.hip: reshape,
    shear_reduce, set_intensity) on the current stream, no host read; the chunk is what fits ``WORKSPACE_BUDGET`` by
    ``perturb_image_bytes``.  The footprints up to ``max_radius`` are built on the host once (seconds at 64).  CPU
    tensors run the statement row by row in the tensor's dtype.

    ``set_width(images, width, intensity=None, bound_frac=.02, validate=False)`` is ``SetWidth`` with ``downscale``, a
    chain of its own (binarise, width, affine_reduce): see its docstring."""

    def __init__(self, scale=16, threshold=.5, seed=0, chunk=None, max_radius=64):
        self.measure = MorphoMeasure(scale, threshold, seed, chunk)
        self.scale, self.threshold, self.seed, self.chunk = self.measure.scale, float(threshold), int(seed), chunk
        self.max_radius = int(max_radius)
        if not 0 <= self.max_radius <= ops.MORPHO_MAX_RADIUS:
            raise ValueError(f"MorphoPerturb: max_radius in 0 .. {ops.MORPHO_MAX_RADIUS}")
        self._rops, self._half, self._ws = {}, {}, {}

    def chunk_for(self, H, W):
        if self.chunk is not None:
            return max(int(self.chunk), 1)
        return max(WORKSPACE_BUDGET // perturb_image_bytes(H, W, self.scale), 1)

    def reduce_operators(self, H, W, device):
        """(RH, RW): the reduce operators as float64 device tensors, built once per size on the host"""
        key = (H, W, str(device))
        if key not in self._rops:
            self._rops[key] = tuple(torch.from_numpy(stmt.reduce_operator(n, self.scale).copy()).to(device)
                                    for n in (H, W)) if self.scale > 1 else (None, None)
        return self._rops[key]

    def half_table(self, device):
        from morphomnist import perturb
        if str(device) not in self._half:
            self._half[str(device)] = torch.from_numpy(perturb.half_width_table(self.max_radius)).to(device)
        return self._half[str(device)]

    def _workspace(self, n, H, W, device):
        need = ops.WS_RESERVED + n * perturb_scratch_bytes(H, W, self.scale)
        ws = self._ws.get(str(device))
        if ws is None or ws.numel() < need:
            ws = self._ws[str(device)] = torch.zeros(need, dtype=torch.uint8, device=device)
        return ws

    @staticmethod
    def _target(t, B, device, dtype, name):
        if t is None:
            return None
        t = torch.as_tensor(t)
        if tuple(t.shape) != (B,) or t.device != device:
            raise ValueError(f"MorphoPerturb: {name} is a [{B}] tensor on {device}, or None")
        return t.to(dtype).contiguous()

    @torch.no_grad()
    def apply(self, images, thickness=None, slant=None, intensity=None):
        s = self.scale
        x, B, H, W = checked_images(images, "MorphoPerturb", s)
        if not x.is_cuda:
            return self._apply_cpu(x, thickness, slant, intensity)
        dev = x.device
        t_t = self._target(thickness, B, dev, torch.float32, "thickness")
        t_i = self._target(intensity, B, dev, torch.float32, "intensity")
        t_s = self._target(slant, B, dev, torch.float64, "slant")
        if t_s is not None:
            t_s = -torch.tan(t_s)                                     # the target shear, fp64 on the device
        out = {"images": torch.empty(B, H, W, dtype=torch.float32, device=dev),
               "status": torch.empty(B, dtype=torch.int32, device=dev),
               "radius": torch.empty(B, dtype=torch.int32, device=dev),
               "thickness_before": torch.empty(B, dtype=torch.float32, device=dev),
               "shear_before": torch.empty(B, dtype=torch.float64, device=dev),
               "intensity_before": torch.empty(B, dtype=torch.float32, device=dev)}
        mm = self.measure
        AH, AW = mm.operators(H, W, dev)
        RH, RW = self.reduce_operators(H, W, dev)
        half = self.half_table(dev)
        n = min(self.chunk_for(H, W), B)
        ws = self._workspace(n, H, W, dev)
        for lo in range(0, B, n):
            hi = min(lo + n, B)
            cut = lambda t: None if t is None else t[lo:hi]
            bits, fg, hstats = ops.morpho_binarise(x[lo:hi], s, AH, AW, self.threshold, ws=ws)
            d2, st = ops.morpho_edt(bits, W * s, ws=ws)
            skel = ops.morpho_thin(bits, d2, fg, st, mm._keep, self.seed, ws=ws)
            _, values, _ = ops.morpho_measure(x[lo:hi], s, skel, d2, fg, hstats, st)
            shaped, radius, sums, st = ops.morpho_reshape(bits, W * s, values[:, 2], cut(t_t), st, half, s, ws=ws)
            q, shear = ops.morpho_shear_reduce(shaped, H, W, s, sums, cut(t_s), st, RH, RW, ws=ws)
            _, median, st = ops.morpho_set_intensity(q, cut(t_i), st, out=out["images"][lo:hi])
            out["status"][lo:hi], out["radius"][lo:hi] = st, radius
            out["thickness_before"][lo:hi], out["shear_before"][lo:hi] = values[:, 2], shear
            out["intensity_before"][lo:hi] = median
        return out

    def _apply_cpu(self, x, thickness, slant, intensity):
        from morphomnist import perturb
        dtype = np.float64 if x.dtype == torch.float64 else np.float32
        B = x.shape[0]
        pick = lambda t, b: None if t is None else torch.as_tensor(t)[b].item()
        rows = [perturb.counterfactual_image(x[b].numpy(), pick(thickness, b), pick(slant, b), pick(intensity, b),
                                             self.scale, self.threshold, self.seed, dtype, self.max_radius)
                for b in range(B)]
        col = lambda k, dt: torch.from_numpy(np.array([r[k] for r in rows], dtype=dt))
        return {"images": torch.from_numpy(np.stack([r["image"] for r in rows]).astype(dtype)),
                "status": col("status", np.int32), "radius": col("radius", np.int32),
                "thickness_before": col("thickness", dtype), "shear_before": col("shear", np.float64),
                "intensity_before": col("median", dtype)}

    # ------------------------------------------------------------------------------------------------- SetWidth
    def width_chunk_for(self, H, W):
        if self.chunk is not None:
            return max(int(self.chunk), 1)
        return max(WORKSPACE_BUDGET // width_image_bytes(H, W, self.scale), 1)

    def _width_workspace(self, n, H, W, device):
        need = ops.WS_RESERVED + n * width_scratch_bytes(H, W, self.scale)
        ws = self._ws.get(str(device))
        if ws is None or ws.numel() < need:
            ws = self._ws[str(device)] = torch.zeros(need, dtype=torch.uint8, device=device)
        return ws

    def _width_round(self, x, H, W, target, frac, operators, ws):
        """binarise, width, affine_reduce of one chunk: (q, status, wb)"""
        AH, AW, RH, RW = operators
        s = self.scale
        bits, fg, _ = ops.morpho_binarise(x, s, AH, AW, self.threshold, ws=ws)
        sums, wb, st = ops.morpho_width(x, s, bits, fg, target, AH, AW, frac, ws=ws)
        q, st = ops.morpho_affine_reduce(bits, H, W, s, sums, wb, st, RH, RW, ws=ws)
        return q, st, wb

    @torch.no_grad()
    def set_width(self, images, width, intensity=None, bound_frac=.02, validate=False):
        """``SetWidth(width)`` and ``downscale`` of ``morphomnist.perturb.width_image`` for a batch, then the scripts'
        intensity rescale when ``intensity`` is given.  ``images`` as ``apply`` takes them; ``width``, ``intensity``: [B]
        tensors on the images' device (``intensity`` may be None), the target width in pixels of the image (the
        ``width`` column ``MorphoMeasure(bound_frac=...)`` measures).

        Returns {"images": float [B, H, W] in 0 .. 255, "status": int32 [B] (0; 1: no background; 4: nothing left to
        work with -- an empty bitmap, every pixel in one row, no grey mass, a width that is not finite or <= 0, or a
        result that is 0 everywhere; 5: the target is NaN, infinite or <= 0 -- the image is 0 then), "width_before":
        float32 [B], the measured width (right - left) / scale, "factor": float64 [B] = width_before / width,
        "bounds_before": float64 [B, 2] = left, right in up-sampled pixels, "shear_before": float64 [B], u11 / u02 of
        the bitmap, "intensity_before": the median of the quantised result (NaN when ``intensity`` is None on a GPU:
        the launch that selects it runs only with a target)}; NaN where the status is not 0.

        ``validate``: the reference's check, once: "width_after" (float32 [B], the width of the first round's result,
        before any intensity rescale, under its own grey moments -- one ``morpho_bounds`` launch) and "off_target" (bool
        [B], |width_after - width| > 1, compared in fp64) are added,
        a second round is computed from the result for the whole chunk and taken, row by row, where the first is off
        target.  Exactly one re-application is made (the reference's ``SetWidth`` recurses until the width fits); the
        outputs named "..._before" stay those of the first round.

        CUDA tensors: per chunk binarise, width, affine_reduce (csrc/morpho.hip) and, only with ``intensity``,
        set_intensity, on the current stream, no host read (``validate``: bounds and the three again); the chunk is
        what fits ``WORKSPACE_BUDGET`` by ``width_image_bytes``.  CPU tensors run the statement row by row in the
        tensor's dtype."""
        s = self.scale
        x, B, H, W = checked_images(images, "MorphoPerturb", s)
        frac = float(bound_frac)
        if not 0.0 < frac < 1.0:
            raise ValueError(f"MorphoPerturb: 0 < bound_frac < 1, got {bound_frac}")
        if width is None:
            raise ValueError(f"MorphoPerturb: width is a [{B}] tensor on {x.device}")
        t_w = self._target(width, B, x.device, torch.float64, "width")
        t_i = self._target(intensity, B, x.device, torch.float32, "intensity")
        if not x.is_cuda:
            return self._set_width_cpu(x, t_w, t_i, frac, validate)
        dev = x.device
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
        out = {"images": f32(B, H, W), "status": torch.empty(B, dtype=torch.int32, device=dev), "width_before": f32(B),
               "factor": f64(B), "bounds_before": f64(B, 2), "shear_before": f64(B),
               "intensity_before": torch.full((B,), float("nan"), dtype=torch.float32, device=dev)}
        if validate:
            out["width_after"], out["off_target"] = f32(B), torch.empty(B, dtype=torch.bool, device=dev)
        operators = (*self.measure.operators(H, W, dev), *self.reduce_operators(H, W, dev))
        n = min(self.width_chunk_for(H, W), B)
        ws = self._width_workspace(n, H, W, dev)
        for lo in range(0, B, n):
            hi = min(lo + n, B)
            q, st, wb = self._width_round(x[lo:hi], H, W, t_w[lo:hi], frac, operators, ws)
            if validate:
                bounds = ops.morpho_bounds(q, s, operators[0], operators[1], frac, ws=ws)
                after = (bounds[:, 1] - bounds[:, 0]) / float(s)
                off = (after - t_w[lo:hi]).abs() > 1.0                # (fp64; a NaN width: not off target)
                q2, st2, _ = self._width_round(q, H, W, t_w[lo:hi], frac, operators, ws)
                q, st = torch.where(off[:, None, None], q2, q), torch.where(off, st2, st)
                out["width_after"][lo:hi], out["off_target"][lo:hi] = after, off
            if t_i is not None:
                _, median, st = ops.morpho_set_intensity(q, t_i[lo:hi], st, out=out["images"][lo:hi])
                out["intensity_before"][lo:hi] = median
            else:
                out["images"][lo:hi] = q
            out["status"][lo:hi] = st
            out["width_before"][lo:hi] = ((wb[:, 1] - wb[:, 0]) / float(s)).float()
            out["factor"][lo:hi], out["bounds_before"][lo:hi], out["shear_before"][lo:hi] = wb[:, 5], wb[:, :2], wb[:, 2]
        return out

    def _set_width_cpu(self, x, width, intensity, frac, validate):
        from morphomnist import perturb
        dtype = np.float64 if x.dtype == torch.float64 else np.float32
        pick = lambda t, b: None if t is None else t[b].item()
        rows = [perturb.width_image(x[b].numpy(), pick(width, b), pick(intensity, b), self.scale, self.threshold, dtype,
                                    frac, validate) for b in range(x.shape[0])]
        first = [r.get("first", r) for r in rows]
        col = lambda rs, k, dt: torch.from_numpy(np.array([r[k] for r in rs], dtype=dt))
        out = {"images": torch.from_numpy(np.stack([r["image"] for r in rows]).astype(dtype)),
               "status": col(rows, "status", np.int32), "width_before": col(first, "source_width", dtype),
               "factor": col(first, "factor", np.float64),
               "bounds_before": torch.stack([col(first, "left", np.float64), col(first, "right", np.float64)], 1),
               "shear_before": col(first, "shear", np.float64), "intensity_before": col(rows, "median", dtype)}
        if validate:
            out["width_after"], out["off_target"] = col(rows, "width_after", dtype), col(rows, "off_target", bool)
        return out


KINDS = ops.MORPHO_KINDS
LOCAL_KEYS = ("images", "bits", "status", "radius", "thickness_before", "n_candidates", "fallback", "centres",
              "endpoints")


def local_image_bytes(H, W, scale):
    """what one image of a ``MorphoLocal`` chunk holds on the device: ``perturb_image_bytes`` and the complement bitmap
    with its distance map"""
    Hh, Wh = H * scale, W * scale
    return perturb_image_bytes(H, W, scale) + 4 * Hh * Wh + 4 * Hh * ((Wh + 31) // 32)


class MorphoLocal:
    """The five Morpho-MNIST data sets' perturbations for a batch: plain, ``Thinning``, ``Thickening``, ``Swelling`` and
    ``Fracture`` of ``morphomnist.perturb`` with ``ImageMorphology.downscale`` (``morphomnist.perturb.local_image``).

    ``apply(images, kind)`` takes images as ``MorphoMeasure.measure`` does and ``kind``: one of ``KINDS`` ("plain",
    "thin", "thick", "swell", "fracture") for the whole batch, or an int32 [B] tensor of kind numbers 0 .. 4 on the
    images' device, one perturbation per image (a number outside 0 .. 4 gives that image status 4; the tensor is not
    read on the host).  Returns {"images": float [B, H, W] in 0 .. 255, "bits": the perturbed bitmaps' words int32 [B, H
    s, ceil(W s / 32)], "status": int32 [B] (0; 1, 2 as ``MorphoMeasure``; 4: nothing left -- no skeleton for any kind
    but plain, or an empty result; the image is 0 then), "radius": int32 [B] (the disk radius of thin / thick /
    fracture, int(R) of a swelling), "thickness_before", "n_candidates": int32 [B] (the skeleton pixels the locations
    were drawn from), "fallback": int32 [B] (1: pruning left none), "centres": int32 [B, 8, 2] (row, column; -1 where
    unused), "endpoints": int32 [B, 8, 4] (r0, c0, r1, c1 of the cuts)}.

    The locations are draws of the counter RNG ("locate" stream of ``ali_hip.rng``) under (seed, counter, global row):
    the counter starts at 0 and advances once per ``apply``, so a fresh executor with the same seed repeats them and
    chunking does not change them.

    CUDA tensors: per chunk the four launches of ``MorphoMeasure``, then locate, local and shear_reduce (csrc/
    morpho.hip), and for "thick" or a kind tensor the complement and its distance map in front of local; on the current
    stream, no host read.  CPU tensors run the statement row by row in the tensor's dtype."""

    def __init__(self, scale=16, threshold=.5, seed=0, chunk=None, thin_amount=.7, thick_amount=1., swell_strength=3.,
                 swell_radius=7., frac_thickness=1.5, frac_prune=2., num_frac=3):
        from morphomnist import perturb
        from morphomnist.skeleton import prune_radius
        self.measure = MorphoMeasure(scale, threshold, seed, chunk)
        self.scale, self.threshold, self.seed, self.chunk = self.measure.scale, float(threshold), int(seed), chunk
        if int(num_frac) != num_frac or not 1 <= int(num_frac) <= ops.MORPHO_MAX_DRAWS:
            raise ValueError(f"MorphoLocal: num_frac in 1 .. {ops.MORPHO_MAX_DRAWS}")
        if not float(swell_strength) >= 1:
            raise ValueError("MorphoLocal: swell_strength >= 1")
        if not (float(thin_amount) >= 0 and float(thick_amount) >= 0 and float(swell_radius) >= 0
                and float(frac_thickness) >= 0 and (frac_prune is None or float(frac_prune) >= 0)):
            raise ValueError("MorphoLocal: the amounts, swell_radius, frac_thickness and frac_prune are >= 0")
        self.params = dict(thin_amount=float(thin_amount), thick_amount=float(thick_amount),
                           swell_strength=float(swell_strength), swell_radius=float(swell_radius),
                           frac_thickness=float(frac_thickness), frac_prune=frac_prune, num_frac=int(num_frac))
        self.frac_radius = perturb.fracture_radius(frac_thickness, self.scale)
        if self.frac_radius > ops.MORPHO_MAX_STAMP:
            raise ValueError(f"MorphoLocal: a fracture brush of radius {self.frac_radius} exceeds {ops.MORPHO_MAX_STAMP}")
        self.prune = prune_radius(frac_prune, self.scale)
        self.calls = 0                                               # the counter of the CPU path
        self._rops, self._ws, self._ctr = {}, {}, {}

    def chunk_for(self, H, W):
        if self.chunk is not None:
            return max(int(self.chunk), 1)
        return max(WORKSPACE_BUDGET // local_image_bytes(H, W, self.scale), 1)

    reduce_operators = MorphoPerturb.reduce_operators
    _workspace = MorphoPerturb._workspace

    def counter(self, device):
        """the device counter (int64 [1]): the number of ``apply`` calls on ``device`` so far"""
        if str(device) not in self._ctr:
            self._ctr[str(device)] = torch.zeros(1, dtype=torch.int64, device=device)
        return self._ctr[str(device)]

    @torch.no_grad()
    def apply(self, images, kind):
        s = self.scale
        x, B, H, W = checked_images(images, "MorphoLocal", s)
        if isinstance(kind, str):
            if kind not in KINDS:
                raise ValueError(f"MorphoLocal: kind is one of {KINDS} or an int32 [B] tensor, got {kind!r}")
            kinds = torch.full((B,), KINDS.index(kind), dtype=torch.int32, device=x.device)
        else:
            if not (torch.is_tensor(kind) and tuple(kind.shape) == (B,) and kind.device == x.device
                    and kind.dtype == torch.int32):
                raise ValueError(f"MorphoLocal: kind is one of {KINDS} or an int32 [{B}] tensor on {x.device}")
            kinds = kind.contiguous()
        if not x.is_cuda:
            return self._apply_cpu(x, kinds)
        dev = x.device
        Hh, Wh = H * s, W * s
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
        out = {"images": torch.empty(B, H, W, dtype=torch.float32, device=dev), "bits": i32(B, Hh, (Wh + 31) // 32),
               "status": i32(B), "radius": i32(B), "thickness_before": torch.empty(B, dtype=torch.float32, device=dev),
               "n_candidates": i32(B), "fallback": i32(B), "centres": i32(B, ops.MORPHO_MAX_DRAWS, 2),
               "endpoints": i32(B, ops.MORPHO_MAX_DRAWS, 4)}
        mm = self.measure
        AH, AW = mm.operators(H, W, dev)
        RH, RW = self.reduce_operators(H, W, dev)
        ctr = self.counter(dev)
        thicken = not isinstance(kind, str) or kind == "thick"
        p = self.params
        n = min(self.chunk_for(H, W), B)
        ws = self._workspace(n, H, W, dev)
        for lo in range(0, B, n):
            hi = min(lo + n, B)
            bits, fg, hstats = ops.morpho_binarise(x[lo:hi], s, AH, AW, self.threshold, ws=ws)
            d2, st = ops.morpho_edt(bits, Wh, ws=ws)
            skel = ops.morpho_thin(bits, d2, fg, st, mm._keep, self.seed, ws=ws)
            _, values, _ = ops.morpho_measure(x[lo:hi], s, skel, d2, fg, hstats, st)
            n_cand, fb, ce, en = ops.morpho_locate(skel, d2, st, kinds[lo:hi], s, self.prune, self.prune, p["num_frac"],
                                                   self.seed, ctr, offset=lo)
            d2c = ops.morpho_edt(ops.morpho_complement(bits, Wh), Wh, ws=ws)[0] if thicken else None
            new, radius, sums, st = ops.morpho_local(bits, Wh, d2, d2c, values[:, 2], st, kinds[lo:hi], n_cand, ce, en, s,
                                                     p["thin_amount"], p["thick_amount"], p["swell_strength"],
                                                     p["swell_radius"], self.frac_radius, p["num_frac"])
            q, _ = ops.morpho_shear_reduce(new, H, W, s, sums, None, st, RH, RW, ws=ws)
            for k, v in (("images", q), ("bits", new), ("status", st), ("radius", radius),
                         ("thickness_before", values[:, 2]), ("n_candidates", n_cand), ("fallback", fb), ("centres", ce),
                         ("endpoints", en)):
                out[k][lo:hi] = v
        ctr += 1
        return out

    def _apply_cpu(self, x, kinds):
        from morphomnist import perturb
        dtype = np.float64 if x.dtype == torch.float64 else np.float32
        rows = [perturb.local_image(x[b].numpy(), int(kinds[b]), self.scale, self.threshold, self.seed, dtype, self.calls,
                                    b, **self.params) for b in range(x.shape[0])]
        self.calls += 1
        col = lambda k, dt: torch.from_numpy(np.array([r[k] for r in rows], dtype=dt))
        return {"images": torch.from_numpy(np.stack([r["image"] for r in rows]).astype(dtype)),
                "bits": pack_bits(np.stack([r["bitmap"] for r in rows])), "status": col("status", np.int32),
                "radius": col("radius", np.int32), "thickness_before": col("thickness", dtype),
                "n_candidates": col("n_candidates", np.int32), "fallback": col("fallback", np.int32),
                "centres": col("centres", np.int32), "endpoints": col("endpoints", np.int32)}
