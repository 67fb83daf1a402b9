"""Drop-in for the reference's ``morphomnist`` package: the measurement half (``morpho``).  ``perturb``, ``skeleton``,
``io`` and the data-set builders are out of scope."""
