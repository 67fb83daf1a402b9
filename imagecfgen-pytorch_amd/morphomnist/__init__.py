"""Drop-in for the reference's ``morphomnist`` package: the measurement half (``morpho``), of ``perturb``
``SetThickness`` / ``SetSlant`` / ``SetIntensity`` with ``ImageMorphology.downscale`` and the four classic
perturbations ``Thinning`` / ``Thickening`` / ``Swelling`` / ``Fracture``, and ``skeleton`` (``LocationSampler``,
``get_angle``) behind them.  ``SetWidth``, ``bounding_parallelogram``, ``measure``'s DataFrame, ``io`` and the
data-set builders are out of scope."""
