"""FiniteVolumeTransport (reference: fv3core/pace/fv3core/stencils/fvtp2d.py:122-346)."""
import ctypes as C

from ._common import Operator, check_layout, dptr
from .delnflux import DelnFlux


class FiniteVolumeTransport(Operator):
    def __init__(self, stencil_factory, quantity_factory, grid_data, damping_coefficients, grid_type: int, hord,
                 nord=None, damp_c=None):
        super().__init__(stencil_factory, quantity_factory, grid_data)
        assert grid_type < 3
        if hord not in (5, 6, 8):
            raise NotImplementedError(f"hord={hord}: implemented on device are the unlimited PPM (5, 6) and the monotone one (8)")
        self._hord = int(hord)
        self._nlev = self.grid_indexing.domain[2]
        self._do_delnflux = (nord is not None) and (damp_c is not None)
        if self._do_delnflux:
            self.delnflux = DelnFlux(stencil_factory, quantity_factory, damping_coefficients, grid_data.rarea, nord, damp_c,
                                     grid_data=grid_data)

    def __call__(self, q, crx, cry, x_area_flux, y_area_flux, q_x_flux, q_y_flux, x_mass_flux=None, y_mass_flux=None,
                 mass=None, levels=None):
        """levels = (k0, nlev): the run of levels k0 .. k0 + nlev - 1 only -- a level's transport depends on that level alone and
        levels are the slowest storage axis, so the run is the same launch with every field pointer advanced by k0 level strides
        (TracerAdvection's Courant-number sub-cycling).  None: all levels."""
        check_layout(self._geom, q, crx, cry, x_area_flux, y_area_flux, q_x_flux, q_y_flux, x_mass_flux, y_mass_flux, mass)
        k0, nlev = 0, self._nlev
        if levels is not None:
            k0, nlev = int(levels[0]), int(levels[1])
            if k0 < 0 or nlev < 1 or k0 + nlev > self._nlev:
                raise ValueError(f"levels = {levels}: a run within the {self._nlev} levels")
            if self._do_delnflux:
                raise NotImplementedError("a run of levels with delnflux damping")
        skip = k0 * self._geom.sk * self._qf.itemsize

        def at(x):
            p = dptr(x)
            return p if p is None else p + skip

        self.call("pace_fvtp2d", C.byref(self._met), at(q), at(crx), at(cry), at(x_area_flux), at(y_area_flux),
                  at(q_x_flux), at(q_y_flux), at(x_mass_flux), at(y_mass_flux), self._hord, nlev, self.stream())
        if self._do_delnflux:
            self.delnflux(q, q_x_flux, q_y_flux, mass=mass)
