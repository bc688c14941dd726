"""stencils/pace/stencils/c2l_ord.py: CubedToLatLon lives in pace_amd.fv3core.stencils.c2l_ord and is re-exported here."""
from ..fv3core.stencils.c2l_ord import CubedToLatLon  # noqa: F401
