"""AGrid2DGridPhysics -- the Fortran update_dwinds_phys (reference: stencils/pace/stencils/update_dwind_phys.py:152-653): the
A-grid wind tendencies u_dt, v_dt applied to the D-grid winds u, v.

One call is pace_update_dwinds_phys: the wind kernel, which recomputes the three-component vector of each of the up to six
A-grid points an output point depends on instead of the reference's twelve scratch fields, followed on the same stream by the
launch that zeroes u_dt, v_dt on the compute domain plus one point."""
import ctypes as C

from ._common import Operator, check_layout, dptr, need_3d, refuse_other_layouts
from ..fv3core.stencils.fillz import pointer_table


class AGrid2DGridPhysics(Operator):
    """Fortran name is update_dwinds_phys"""

    def __init__(self, stencil_factory, quantity_factory, partitioner, rank: int, namelist, grid_info):
        """The reference's arguments (:157-165); partitioner and rank only matter for layouts other than (1, 1), which are
        refused."""
        refuse_other_layouts(namelist)
        qf = quantity_factory if quantity_factory is not None else stencil_factory.quantity_factory
        if qf is None:
            raise ValueError("AGrid2DGridPhysics needs the field layout: a quantity factory")
        super().__init__(stencil_factory, qf)
        n = self._geom.n
        if (namelist.npx, namelist.npy) != (n + 1, n + 1):
            raise ValueError(f"namelist npx, npy = {namelist.npx}, {namelist.npy} do not match the {n} x {n} tile")
        if n % 2 or n < 4:
            raise ValueError("the edge vectors need an even tile size of at least 4 (geometry.py:726-729)")
        self.namelist = namelist
        self._dt5 = 0.5 * self.namelist.dt_atmos
        self._im2 = int((namelist.npx - 1) / 2) + 2
        self._jm2 = int((namelist.npy - 1) / 2) + 2
        self._grid_info = grid_info
        gi = grid_info
        self._vectors = [pointer_table([getattr(gi, f"{name}{m}") for m in (1, 2, 3)])
                         for name in ("vlon", "vlat", "es1_", "ew2_")]
        self._edges = [gi.edge_vect_w, gi.edge_vect_e, gi.edge_vect_s, gi.edge_vect_n]
        for e in self._edges:
            if e.dim() != 1 or e.shape[0] != n + 7 or e.dtype != qf.real or e.device.type != qf.device.type:
                raise ValueError("edge_vect_*: 1-D tensors of nx + 7 entries of the library's storage type, on its device")

    def __call__(self, u, v, u_dt, v_dt):
        """Transforms the wind tendencies from A grid to D grid for the final update.

        u, v (inout): D-grid winds; u_dt, v_dt (inout): A-grid tendencies with their one-point halo updated, zero afterwards
        on the compute domain plus one point."""
        need_3d("AGrid2DGridPhysics", u, v, u_dt, v_dt)
        check_layout(self._geom, u, v, u_dt, v_dt)
        self.call("pace_update_dwinds_phys", dptr(u), dptr(v), dptr(u_dt), dptr(v_dt), *self._vectors,
                  *[C.c_void_p(e.data_ptr()) for e in self._edges], self._dt5, self.stream())
