"""What the end-of-step operators share."""
from ..fv3core.stencils._common import Operator, check_layout, dptr  # noqa: F401


def refuse_other_layouts(namelist):
    layout = tuple(getattr(namelist, "layout", (1, 1)))
    if layout != (1, 1):
        raise NotImplementedError(f"layout {layout}: pace_amd maps one cubed-sphere tile per device, layout must be (1, 1)")


class _Addressed:
    """A bare tensor as the halo updaters take their fields: `ptr` is the address of element (0, 0, 0)."""

    generation = 0

    def __init__(self, tensor):
        self.data = tensor
        self.ptr = tensor.data_ptr()


def addressed(field):
    """A Quantity as it is; a tensor of the library's layout wrapped so that a halo updater can be started on it."""
    return field if hasattr(field, "ptr") else _Addressed(field)


class AddressedState:
    """A state namespace whose fields may be tensors, seen through `addressed`."""

    def __init__(self, state):
        self._state = state

    def __getattr__(self, name):
        return addressed(getattr(self._state, name))


def need_3d(owner, *fields):
    for f in fields:
        if f is None:
            raise ValueError(f"{owner} needs every field of its call")
        t = f.data if hasattr(f, "dims") else f
        if t.dim() != 3:
            raise ValueError(f"field of shape {tuple(t.shape)}: {owner} takes 3-D fields")
