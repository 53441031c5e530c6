"""Host-side mirror of the reference's robust GP class (models/GP_Robust.py) on the MI355X sweep engine.

models/GP_Robust.py is models/GP_Safe.py with two differences, and so is this class:
  * the prior mean is zero for every output (models/GP_Robust.py:322-324; GP_Safe uses -2 Y_mean / Y_std for the constraints) --
    uploaded with ``sbo_model_set_prior``;
  * the lower bound of log sigma_n in the hyper-parameter fit is -8 instead of -5 (models/GP_Robust.py:205), in every fit path
    (SciPy DE on the host, ``fit_on_device`` True / "de").
The inputs are x = concat(xc, d): the disturbance coordinates are the last input axes.
"""
from __future__ import annotations

from .GP_Safe import GP as _GPSafe


class GP(_GPSafe):
    noise_lower_bound = -8.0
    mean_prior_zero = True
