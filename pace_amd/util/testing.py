"""pace.util.testing.perturb (util/pace/util/testing/perturbation.py): the roundoff perturbation of the checkpoint tests."""
from typing import Mapping

import numpy as np
import torch


def perturb(input: Mapping, generator=None):
    """
    Adds roundoff-level noise to the input array in-place through multiplication.

    Will only make changes to float type arrays: float tensors and numpy arrays, and the `data` of a Quantity on its device.
    Values of 1e30 and above are left as they are.  generator: a torch.Generator (tensors) or a numpy Generator (arrays), so
    that a run is repeatable; a torch.Generator lives on the device of the tensors it serves.
    """
    roundoff = 1e-16
    for data in input.values():
        if hasattr(data, "dims"):
            data = data.data
        if torch.is_tensor(data):
            if data.is_floating_point():
                gen = generator if isinstance(generator, torch.Generator) else None
                noise = torch.rand(data.shape, dtype=torch.float64, device=data.device, generator=gen)
                factor = (1.0 + (2.0 * noise - 1.0) * roundoff).to(data.dtype)
                data.mul_(torch.where(data < 1e30, factor, torch.ones_like(factor)))
        elif isinstance(data, np.ndarray) and np.issubdtype(data.dtype, np.floating):
            rng = generator if isinstance(generator, np.random.Generator) else np.random.default_rng()
            not_fill_value = data < 1e30
            # multiply data by roundoff-level error
            data[not_fill_value] *= 1.0 + rng.uniform(low=-roundoff, high=roundoff, size=data[not_fill_value].shape)
