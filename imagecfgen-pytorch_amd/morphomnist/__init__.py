"""Drop-in for the reference's ``morphomnist`` package: the measurement half (``morpho``) and, of ``perturb``,
``SetThickness`` / ``SetSlant`` / ``SetIntensity`` / ``Thinning`` / ``Thickening`` with ``ImageMorphology.downscale``
(DESIGN 3.17).  ``Swelling``, ``Fracture``, ``SetWidth``, ``skeleton``, ``io`` and the data-set builders are out of scope
(DESIGN 7)."""
