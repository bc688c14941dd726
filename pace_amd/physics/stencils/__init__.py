from . import microphysics  # noqa: F401
