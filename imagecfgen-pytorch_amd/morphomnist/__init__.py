"""Drop-in for the reference's ``morphomnist`` package: the measurement half (``morpho``, with
``bounding_parallelogram``), ``measure`` (``Morphometrics``, ``measure_image``, ``measure_batch``'s DataFrame; DESIGN
3.21), of ``perturb`` ``SetThickness`` / ``SetSlant`` / ``SetIntensity`` with ``ImageMorphology.downscale``
and the four classic perturbations ``Thinning`` / ``Thickening`` / ``Swelling`` / ``Fracture``, and ``skeleton``
(``LocationSampler``, ``get_angle``) behind them.  ``SetWidth``, ``io`` and the data-set builders are out
of scope."""
