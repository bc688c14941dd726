"""Gather and scatter across the cube: the other half of the reference communicator's public interface
(util/pace/util/communicator.py:111-329, 734-772) for layout (1, 1), where the "subtiles" of the global array are the six tiles.

The device side is ``pace_cube_gather`` / ``pace_cube_scatter`` (pace_amd/csrc/k_gather.hip): one launch moves the compute
domains of any number of fields of any of the six tiles between their storages and ONE dense buffer in the reference's axis
order.  What a call costs depends on the transport:

* ``DeviceCubeComm`` (``run_cube``): the six ranks meet (``ThreadComm.rendezvous``), and the last to arrive builds the table of
  all tiles and all variables of the call -- cached on the device per set of addresses, uploaded through a pinned array like the
  halo tables -- and launches ONCE.  ``gather_state`` adds ONE transfer of the whole state to a pinned host buffer.
* ``ThreadComm`` and ``run_cube(snapshot=True)``: the ranks meet to share the dense buffer, then every rank launches for its own
  tile (one launch per rank).
* ``TorchDistComm``: every rank packs its tile with one launch, then ``torch.distributed.gather`` / ``scatter`` moves the dense
  tensors; names, metadata and ``time`` go through ``broadcast_object_list``.
* ``NullComm``: the rank's own slot holds its data, the other five the comm's fill value.

The dense layout of a call is field-major: variable f of tile r lies at ``6 * off[f] + r * size[f]`` elements, so that every
variable's ``(6,) + extent`` array is one contiguous block (the file writers take it as it is).  Under ``TorchDistComm`` the
buffer the collective fills is rank-major and a variable's array is a strided view of it.
"""
import collections
import ctypes as C

import numpy as np
import torch

from .. import _launch, _lib
from . import constants as c
from .quantity import Quantity, QuantityFactory, SubtileGridSizer

CUBE_TILE_I, CUBE_TILE_S = 64, 32  # pace_amd/csrc/wgmap.h WT_TI, WT_TS (tests/test_cube_gather.py holds them together)
TABLE_CACHE = 8  # device tables kept per communicator
_TORCH_OF = {np.dtype("float64"): torch.float64, np.dtype("float32"): torch.float32}

Meta = collections.namedtuple("Meta", "name dims extent units dtype")  # extent: of ONE tile; dtype: a torch dtype


# ---------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------
def cube_tiles(item) -> int:
    """Workgroup tiles of one item (include/pace_hip.h: the prefix table behind the items counts these)."""
    volume = item.kind == _lib.DIAG_WINDOW3D
    ns = item.nk if volume else item.nj
    per = -(-item.ni // CUBE_TILE_I) * -(-ns // CUBE_TILE_S)
    return per * item.nj if volume else per


def check_cube_items(geom, items, scatter=False):
    """The host checks of a pace_cube_gather / pace_cube_scatter table, before any launch (the entry point sees device memory
    only): the count, every window non-empty and inside its field's storage ((n + 7)^2 points, nk + 1 levels), no NULL field, no
    negative offset; for scatter, no two items that overlap on one field (the result would depend on the order of the
    workgroups).  Raises ValueError."""
    if len(items) < 1 or len(items) > _lib.CUBE_MAX_ITEMS:
        raise ValueError(f"a cube table holds 1 .. {_lib.CUBE_MAX_ITEMS} items, not {len(items)}")
    ni, nlev = geom.n + 7, geom.nk + 1
    written = collections.defaultdict(list)
    tiles = 0
    for t, x in enumerate(items):
        if x.kind not in (_lib.DIAG_WINDOW3D, _lib.DIAG_PLANE):
            raise ValueError(f"cube table item {t}: kind {x.kind} is neither a 3-D window nor a plane")
        if not x.field:
            raise ValueError(f"cube table item {t}: null field")
        if x.offset < 0:
            raise ValueError(f"cube table item {t}: negative offset {x.offset}")
        if x.ni < 1 or x.nj < 1 or x.nk < 1:
            raise ValueError(f"cube table item {t}: empty window {(x.ni, x.nj, x.nk)}")
        if x.kind == _lib.DIAG_PLANE and (x.k0 != 0 or x.nk != 1):
            raise ValueError(f"cube table item {t}: a plane has k0 = 0 and nk = 1")
        if min(x.i0, x.j0, x.k0) < 0 or x.i0 + x.ni > ni or x.j0 + x.nj > ni or x.k0 + x.nk > nlev:
            raise ValueError(f"cube table item {t}: the window {(x.i0, x.j0, x.k0)} + {(x.ni, x.nj, x.nk)} lies outside the "
                             f"field's storage of {ni} x {ni} x {nlev} points")
        if scatter:
            for u, y in written[x.field]:
                if (x.i0 < y.i0 + y.ni and y.i0 < x.i0 + x.ni and x.j0 < y.j0 + y.nj and y.j0 < x.j0 + x.nj
                        and x.k0 < y.k0 + y.nk and y.k0 < x.k0 + x.nk):
                    raise ValueError(f"cube table items {u} and {t} overlap on one field")
            written[x.field].append((t, x))
        tiles += cube_tiles(x)
    if tiles >= 2 ** 31:
        raise ValueError(f"{tiles} tiles in one cube table")


def build_cube_table(geom, items, scatter=False):
    """The bytes of a table as the kernels read it: the items, then int32 first[n + 1], the prefix sums of their tile counts
    (padded to 8-byte units for the upload).  Checks the items first."""
    check_cube_items(geom, items, scatter)
    n = len(items)
    item_bytes = C.sizeof(_lib.CubeItem) * n
    buf = (C.c_uint8 * ((item_bytes + 4 * (n + 1) + 7) // 8 * 8))()
    C.memmove(buf, (_lib.CubeItem * n)(*items), item_bytes)
    first = np.zeros(n + 1, dtype=np.int32)
    first[1:] = np.cumsum([cube_tiles(x) for x in items])
    C.memmove(C.addressof(buf) + item_bytes, first.ctypes.data, first.nbytes)
    return buf


def geom_of(quantities):
    """The one geometry of the fields of a call: the first 3-D field gives the levels, a later one may have fewer."""
    def refuse(q):
        return f"gather and scatter move (x, y) and (x, y, z) fields, not {q.dims}"

    for q in quantities:
        if len(q.dims) not in (2, 3) or q.dims[0] not in c.X_DIMS or q.dims[1] not in c.Y_DIMS:
            raise ValueError(refuse(q))
    return _launch.geometry(quantities, refuse, "the fields of one gather or scatter differ in geometry", fewer_levels=True)


class Window:
    """A window of a field other than its compute domain, where gather and gather_state take a Quantity: one level's plane
    (the diagnostics' z_select), or any box of the storage.  `window` is (i0, j0, k0, ni, nj, nk); a PLANE has k0 = 0, nk = 1
    and `level` names its plane; `dims` and `units` are those of the gathered array."""

    def __init__(self, quantity, kind, level, window, dims, units):
        self.data, self.shape, self.kind, self.window = quantity.data, quantity.shape, kind, tuple(window)
        self.ptr = _launch.window_of(quantity, level or None, window)[0]
        self.dims, self.units = tuple(dims), units
        self.origin = self.window[:len(self.dims)]
        self.extent = self.window[3:3 + len(self.dims)]


def item_of(q, offset):
    """The compute domain of a field (interface points included), or a Window, as one item at `offset` elements of the dense
    buffer."""
    x = _lib.CubeItem()
    _launch.set_window(x, (q.ptr, q.kind) + q.window if isinstance(q, Window) else _launch.window_of(q))
    x.offset = int(offset)
    return x


def _size(extent):
    return int(np.prod(extent, dtype=np.int64))


def _meta_of(name, q):
    return Meta(name, tuple(q.dims), tuple(q.extent), q.units, q.data.dtype)


def _dense_code(dtype):
    if dtype == torch.float64:
        return _lib.DENSE_F64
    if dtype == torch.float32:
        return _lib.DENSE_F32
    raise ValueError(f"the dense side of a gather or scatter is float64 or float32, not {dtype}")


class _Layout:
    """Where variable f of tile r lies in the dense buffer of a call."""

    def __init__(self, metas, ranks, rank_major=False):
        self.metas = list(metas)
        self.sizes = [_size(m.extent) for m in self.metas]
        self.offs = [0] + list(np.cumsum(self.sizes)[:-1])
        self.per_rank = int(sum(self.sizes))
        self.ranks, self.rank_major = ranks, rank_major
        self.total = self.per_rank * ranks

    def offset(self, f, r):
        if self.rank_major:
            return r * self.per_rank + int(self.offs[f])
        return self.ranks * int(self.offs[f]) + r * self.sizes[f]

    def array(self, flat, f):
        """Variable f's (ranks,) + extent array as a view of the flat buffer (tensor or ndarray)."""
        shape = (self.ranks,) + tuple(self.metas[f].extent)
        if self.rank_major:
            return flat.reshape(self.ranks, self.per_rank)[:, int(self.offs[f]):int(self.offs[f]) + self.sizes[f]].reshape(shape)
        start = self.ranks * int(self.offs[f])
        return flat[start:start + self.ranks * self.sizes[f]].reshape(shape)


class GatherScatter:
    """gather, gather_state, scatter, scatter_state of CubedSphereCommunicator (a mixin: it uses the communicator's comm, lib,
    device, stream() and rank)."""

    quantity_factory = None  # a QuantityFactory to allocate what scatter receives into; by default one is made from the metadata

    # ---- plumbing ---------------------------------------------------------------------------------------------
    def _gs_mode(self):
        comm = self.comm
        if hasattr(comm, "rendezvous"):
            return "cube" if hasattr(comm, "halo_post") and not getattr(comm, "snapshot", False) else "ranks"
        return "dist" if hasattr(comm, "_dist") else "null"

    def _gs_state(self):
        if not hasattr(self, "_gs_tables"):
            self._gs_tables = collections.OrderedDict()  # key -> (tensors that keep the table alive, n, geom)
            self._gs_buffers = {}  # (elements, dtype) -> (device buffer, pinned host buffer) of gather_state / scatter_state
            self._gs_factories = {}
        return self

    def _gs_check_real(self, quantities):
        for q in quantities:
            if q.data.element_size() != self.lib.real_bytes or not q.data.is_floating_point():
                raise ValueError(f"this communicator's library moves float{8 * self.lib.real_bytes} fields, not {q.data.dtype}")

    def _gs_launch(self, scatter, per_rank, layout, dense):
        """ONE launch for the tiles in per_rank = {rank: quantities}; the table is cached per set of addresses."""
        self._gs_state()
        key = (bool(scatter), layout.rank_major, tuple((r, tuple((q.ptr, tuple(q.origin), tuple(q.extent)) for q in qs)) for r, qs in sorted(per_rank.items())),
               tuple(layout.sizes))
        hit = self._gs_tables.get(key)
        if hit is None:
            every = [q for _, qs in sorted(per_rank.items()) for q in qs]
            self._gs_check_real(every)
            geom = geom_of(every)
            slot = 0 if (layout.rank_major and len(per_rank) == 1) else None  # (a rank's own pack under TorchDistComm)
            items = [item_of(q, layout.offset(f, r if slot is None else slot)) for r, qs in sorted(per_rank.items()) for f, q in enumerate(qs)]
            buf = build_cube_table(geom, items, scatter)
            hit = self._gs_tables[key] = (_launch.upload_table(buf, self.device), len(items), geom)
            if len(self._gs_tables) > TABLE_CACHE:
                self._gs_tables.popitem(last=False)
        else:
            self._gs_tables.move_to_end(key)
        keep, n, geom = hit
        self.lib.call("pace_cube_scatter" if scatter else "pace_cube_gather", C.byref(geom), C.c_void_p(keep[0].data_ptr()), n,
                      _dense_code(dense.dtype), C.c_void_p(dense.data_ptr()), self.stream())

    def _gs_stream_id(self):
        return getattr(self.stream(), "value", None)

    def _gs_bcast(self, obj):
        """An object from the root to every rank of a TorchDistComm."""
        box = [obj]
        self.comm._dist.broadcast_object_list(box, src=c.ROOT_RANK, group=self.comm._group)
        return box[0]

    def _gs_factory(self, meta):
        """The factory scatter allocates with: the communicator's, or one for the tile the metadata describes."""
        if self.quantity_factory is not None:
            return self.quantity_factory
        ext = dict(zip(meta.dims, meta.extent))
        nx = ext[c.X_DIM] if c.X_DIM in ext else ext[c.X_INTERFACE_DIM] - 1
        ny = ext[c.Y_DIM] if c.Y_DIM in ext else ext[c.Y_INTERFACE_DIM] - 1
        nz = ext[c.Z_DIM] if c.Z_DIM in ext else ext[c.Z_INTERFACE_DIM] - 1 if c.Z_INTERFACE_DIM in ext else None
        key = (nx, ny, nz, meta.dtype)
        if nz is None:  # a 2-D field: any factory of this tile size serves
            for (kx, ky, _, kd), f in self._gs_state()._gs_factories.items():
                if (kx, ky, kd) == (nx, ny, meta.dtype):
                    return f
            key = (nx, ny, 1, meta.dtype)
        fac = self._gs_state()._gs_factories
        if key not in fac:
            fac[key] = QuantityFactory(SubtileGridSizer(nx, ny, key[2]), self.device, meta.dtype)
        return fac[key]

    def _gs_buffer(self, elements, dtype, what=None):
        """The device buffer and the pinned host buffer of a whole state (kept: the next call of the same size reuses them;
        `what`: a buffer apart from gather_state's of the same size)."""
        buf = self._gs_state()._gs_buffers
        key = (int(elements), dtype) if what is None else (int(elements), dtype, what)
        if key not in buf:
            buf[key] = _launch.staging(elements, dtype, self.device, alias_on_cpu=True)
        return buf[key]

    # ---- gather ------------------------------------------------------------------------------------------------
    def _gs_recv_flat(self, send_quantity, recv_quantity, ranks):
        """The flat dense tensor behind recv_quantity if a launch can write it in place, else None."""
        if recv_quantity is None or not torch.is_tensor(recv_quantity.data):
            return None
        d = recv_quantity.data
        if tuple(d.shape) != (ranks,) + tuple(send_quantity.extent):
            raise ValueError(f"recv_quantity has shape {tuple(d.shape)}, the gathered array {(ranks,) + tuple(send_quantity.extent)}")
        return d.reshape(-1) if d.is_contiguous() and d.device == self.device and d.dtype in (torch.float64, torch.float32) else None

    def gather(self, send_quantity, recv_quantity=None):
        """communicator.py:194-246.  Returns on the root a Quantity of dims (TILE_DIM,) + send.dims, origin all zeros, extent
        (6,) + send.extent -- the compute domain, interface points included -- whose storage is a dense C-ordered tensor on the
        sender's device in the sender's dtype; None on the other ranks.  ``recv_quantity`` (root) is written in place."""
        ranks = self.comm.Get_size()
        mode = self._gs_mode()
        root = self.rank == c.ROOT_RANK or mode == "null"  # (a rank without peers is its own root, as NullComm.Gather answers)
        meta = _meta_of(None, send_quantity)
        inplace = self._gs_recv_flat(send_quantity, recv_quantity, ranks) if root else None
        dtype = inplace.dtype if inplace is not None else meta.dtype
        if mode in ("cube", "ranks"):
            def dense_of(posts, layout):
                given = posts[c.ROOT_RANK]["dense"]
                return given if given is not None else torch.empty(layout.total, dtype=posts[c.ROOT_RANK]["dtype"], device=self.device)

            # (the root's payload carries where the result goes; the other ranks' entries are not read)
            dense, layout = self._gs_gather_meet(("gather",), [send_quantity], {"dense": inplace, "dtype": dtype}, dense_of)
        elif mode == "dist":
            layout = _Layout([meta], ranks, rank_major=True)
            local = torch.empty(layout.per_rank, dtype=dtype, device=self.device)
            self._gs_launch(False, {self.rank: [send_quantity]}, layout, local)
            dense = (inplace if inplace is not None else torch.empty(layout.total, dtype=dtype, device=self.device)) if root else None
            _launch.wait_for(self.device)
            self.comm._dist.gather(local, list(dense.reshape(ranks, -1).unbind(0)) if root else None, dst=c.ROOT_RANK,
                                   group=self.comm._group)
        else:
            layout = _Layout([meta], ranks)
            dense = inplace if inplace is not None else torch.empty(layout.total, dtype=dtype, device=self.device)
            dense.fill_(getattr(self.comm, "_fill_value", 0.0))
            self._gs_launch(False, {self.rank: [send_quantity]}, layout, dense)
        if not root:
            return None
        out = layout.array(dense, 0)
        if recv_quantity is None:
            return Quantity(out, (c.TILE_DIM,) + meta.dims, meta.units, origin=(0,) * (len(meta.dims) + 1), extent=tuple(out.shape))
        if inplace is None:  # a recv_quantity the launch could not write: copy
            if torch.is_tensor(recv_quantity.data):
                recv_quantity.data.copy_(out)
            else:
                _launch.wait_for(self.device)
                np.copyto(recv_quantity.data, out.cpu().numpy())
        return recv_quantity

    def _gs_gather_meet(self, tag, quantities, payload_extra, dense_of, after=None, metas=None):
        """The rendezvous of the thread transports for a gather.  Every rank posts its fields (and payload_extra: the root's says
        where the result goes); ``dense_of(posts, layout)`` runs on the last rank to arrive; under DeviceCubeComm that rank also
        launches for the whole cube and runs ``after(posts, dense)`` (the transfer to the host), otherwise every rank launches for
        its own tile once it knows the buffer.  Returns (dense, layout) on every rank."""
        fused = self._gs_mode() == "cube"
        comm = self.comm

        def last(posts):
            if len({p["stream"] for p in posts.values()}) != 1:
                raise RuntimeError("the tiles of a gather or scatter called it on different streams: the launch is ordered behind one")
            shapes = [[(q.dims, q.extent, q.data.dtype) for q in p["qs"]] for p in posts.values()]
            if any(s != shapes[0] for s in shapes[1:]):
                raise ValueError("the tiles of a gather or scatter hand over different fields")
            layout = _Layout(metas if metas is not None else [_meta_of(None, q) for q in quantities], comm.Get_size())
            dense = dense_of(posts, layout)
            if fused:
                posts[c.ROOT_RANK]["owner"]._gs_launch(False, {r: p["qs"] for r, p in posts.items()}, layout, dense)
                if after is not None:
                    after(posts, dense)
            return dense, layout

        payload = {"qs": list(quantities), "stream": self._gs_stream_id(), "owner": self}
        payload.update(payload_extra)
        dense, layout = comm.rendezvous(tag, payload, last)
        if not fused:
            self._gs_launch(False, {self.rank: list(quantities)}, layout, dense)
            comm.barrier()  # the root reads the buffer only behind every rank's launch
            if after is not None and self.rank == c.ROOT_RANK:
                after({c.ROOT_RANK: payload}, dense)
        return dense, layout

    def gather_state(self, send_state=None, recv_state=None, transfer_type=None):
        """communicator.py:248-281.  ``time`` is copied from the root; ``transfer_type`` (numpy.float32 or numpy.float64; by
        default the fields' own type) is the type of the results.  On the root the values are Quantities of numpy arrays of
        dims (TILE_DIM,) + dims -- views of ONE pinned host buffer that one launch and one transfer fill for the whole state, and
        that THE NEXT CALL OVERWRITES (as GeosDycoreWrapper's outputs are): copy what has to outlive it.  A variable already in
        ``recv_state`` is written in place instead."""
        ranks = self.comm.Get_size()
        mode = self._gs_mode()
        root = self.rank == c.ROOT_RANK or mode == "null"  # (a rank without peers is its own root)
        names = [n for n in send_state if n != "time"]
        qs = [send_state[n] for n in names]
        if root and recv_state is None:
            recv_state = {}
        if root and "time" in send_state:
            recv_state["time"] = send_state["time"]
        if not names:
            return recv_state
        dtype = _TORCH_OF[np.dtype(transfer_type)] if transfer_type is not None else qs[0].data.dtype
        metas = [_meta_of(n, q) for n, q in zip(names, qs)]
        host = None
        if mode in ("cube", "ranks"):
            def dense_of(posts, layout):
                return posts[c.ROOT_RANK]["owner"]._gs_buffer(layout.total, posts[c.ROOT_RANK]["dtype"])[0]

            def after(posts, dense):
                owner = posts[c.ROOT_RANK]["owner"]
                h = owner._gs_buffer(dense.numel(), dense.dtype)[1]
                if h is not dense:
                    h.copy_(dense, non_blocking=True)

            dense, layout = self._gs_gather_meet(("gather_state", tuple(names)), qs, {"dtype": dtype}, dense_of, after, metas)
            if root:
                host = self._gs_buffer(layout.total, dtype)[1]
        elif mode == "dist":
            layout = _Layout(metas, ranks, rank_major=True)
            local = torch.empty(layout.per_rank, dtype=dtype, device=self.device)
            self._gs_launch(False, {self.rank: qs}, layout, local)
            dense, host = self._gs_buffer(layout.total, dtype) if root else (None, None)
            _launch.wait_for(self.device)
            self.comm._dist.gather(local, list(dense.reshape(ranks, -1).unbind(0)) if root else None, dst=c.ROOT_RANK,
                                   group=self.comm._group)
            if root and host is not dense:
                host.copy_(dense, non_blocking=True)
        else:
            layout = _Layout(metas, ranks)
            dense, host = self._gs_buffer(layout.total, dtype)
            dense.fill_(getattr(self.comm, "_fill_value", 0.0))
            self._gs_launch(False, {self.rank: qs}, layout, dense)
            if host is not dense:
                host.copy_(dense, non_blocking=True)
        if not root:
            return recv_state
        _launch.wait_for(self.device)
        flat = host.numpy()
        for f, m in enumerate(metas):
            arr = layout.array(flat, f)
            if m.name in recv_state:
                target = recv_state[m.name]
                if torch.is_tensor(target.data):
                    target.data.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
                else:
                    np.copyto(target.data, arr)
            else:
                recv_state[m.name] = Quantity(arr, (c.TILE_DIM,) + m.dims, m.units, origin=(0,) * (len(m.dims) + 1), extent=arr.shape)
        return recv_state

    # ---- regrid ------------------------------------------------------------------------------------------------
    @staticmethod
    def _rg_to_host(dense, host):
        """The one transfer of a regrid_state call (regrid_state calls it through this name: the one-transfer tests count it
        here); the root waits for it once."""
        if host is not dense:
            host.copy_(dense, non_blocking=True)

    def _rg_points(self, geom, grid, posts):
        """The point table of (geometry, grid) on the device: built from the six ranks' cell centres and uploaded ONCE."""
        from . import latlon

        state = self._gs_state()
        if not hasattr(state, "_rg_tables"):
            state._rg_tables = {}  # (n, nlon, nlat) -> (the tensors that keep the point table alive, npoints)
            state._rg_items = collections.OrderedDict()  # the item tables, cached per set of addresses like gather's
        key = (geom.n, grid.nlon, grid.nlat)
        if key not in state._rg_tables:
            centres = []
            for r in sorted(posts):
                given = posts[r]["centres"]
                if given is None:  # the grid this project generates: a function of (n, tile) alone
                    from . import gridgen

                    terms = gridgen.tiles(geom.n, geom.nk)[r % 6]
                    given = (terms["lon_agrid"], terms["lat_agrid"])
                centres.append([latlon.compute_domain(a, geom.n) for a in given])
            table = latlon.build_regrid_table(np.stack([x[0] for x in centres]), np.stack([x[1] for x in centres]), *grid.targets())
            state._rg_tables[key] = (latlon.upload_points(geom, table, self.device), table.npoints)
        return state._rg_tables[key]

    def _rg_launch(self, posts, names, grid, dtype):
        """On the last rank to arrive, as the root's communicator: the launches and the transfer of one regrid_state call.
        Returns (host buffer, metas)."""
        from . import latlon

        ranks = sorted(posts)
        if len({posts[r]["stream"] for r in ranks}) != 1:
            raise RuntimeError("the tiles of a regrid called it on different streams: the launch is ordered behind one")
        shapes = [[(q.dims, q.extent, q.data.dtype) for q in posts[r]["qs"]] for r in ranks]
        if any(s != shapes[0] for s in shapes[1:]):
            raise ValueError("the tiles of a regrid hand over different fields")
        every = [q for r in ranks for q in posts[r]["qs"]]
        self._gs_check_real(every)
        geom = geom_of(every)
        keep, npoints = self._rg_points(geom, grid, posts)
        specs, metas, offset = [], [], 0
        for f, name in enumerate(names):
            q = posts[ranks[0]]["qs"][f]
            kind, k0, nk = latlon.levels_of(name, q, geom.n)
            if kind == _lib.DIAG_WINDOW3D:
                metas.append(Meta(name, (c.LON_DIM, c.LAT_DIM, c.Z_DIM), (grid.nlon, grid.nlat, nk), q.units, dtype))
            else:
                metas.append(Meta(name, (c.LON_DIM, c.LAT_DIM), (grid.nlon, grid.nlat), q.units, dtype))
            specs.append((tuple(posts[r]["qs"][f].ptr for r in ranks), kind, k0, nk, offset))
            offset += npoints * nk
        dense, host = self._gs_buffer(offset, dtype, "regrid")
        key = (geom.n, grid.nlon, grid.nlat, tuple(specs))  # (the table does not depend on the dense type)
        state = self._gs_state()
        tables = state._rg_items.get(key)
        if tables is not None:
            state._rg_items.move_to_end(key)
        items = [latlon.regrid_item(*spec) for spec in specs] if tables is None else None
        state._rg_items[key] = latlon.launch_regrid(self.lib, geom, keep[0], npoints, items, dense, self.stream(), tables)
        if len(state._rg_items) > TABLE_CACHE:
            state._rg_items.popitem(last=False)
        self._rg_to_host(dense, host)
        return host, metas

    def regrid_state(self, windows, grid, transfer_type=None, centres=None):
        """The state on a regular latitude-longitude grid (this project's extension; pace_amd/util/latlon.py): cell-centre
        fields of all six tiles interpolated on the device and only the lat-lon arrays transferred.

        ``windows``: {name: Quantity with dims (x, y) or (x, y, z), or a gather Window -- one level's plane, or a level range} of
        this rank's tile (``time`` is copied from the root); ``grid``: a LatLonGrid; ``transfer_type``: numpy.float32 or
        numpy.float64 (by default the fields' own type); ``centres``: this tile's (lon_agrid, lat_agrid) [radians], by default
        those of the grid pace_amd.util.gridgen generates.  The table is built once per (geometry, grid) and uploaded once; a
        call is ONE pace_cube_regrid launch per PACE_REGRID_MAX_ITEMS variables, ONE transfer and ONE synchronisation.  On the
        root the values are Quantities of numpy arrays with dims (lon, lat) or (lon, lat, z) -- views of ONE pinned host buffer
        that THE NEXT CALL OVERWRITES, as gather_state's are; None on the other ranks.  Needs the whole cube on one device
        (run_cube, run_cube_driver)."""
        if self._gs_mode() != "cube":
            raise ValueError("regrid_state needs a communicator that holds the whole cube on one device: run the six tiles with "
                             "pace_amd.util.run_cube (the driver: comm_config.type: cube, run_cube_driver)")
        root = self.rank == c.ROOT_RANK
        names = [n for n in windows if n != "time"]
        qs = [windows[n] for n in names]
        if not names:
            return ({"time": windows["time"]} if "time" in windows else {}) if root else None
        dtype = _TORCH_OF[np.dtype(transfer_type)] if transfer_type is not None else qs[0].data.dtype
        from . import latlon

        for name, q in zip(names, qs):  # (every rank refuses its own before the ranks meet)
            latlon.levels_of(name, q, q.data.shape[0] - 2 * c.N_HALO_DEFAULT - 1)

        def last(posts):
            return posts[c.ROOT_RANK]["owner"]._rg_launch(posts, names, grid, posts[c.ROOT_RANK]["dtype"])

        payload = {"qs": qs, "stream": self._gs_stream_id(), "owner": self, "centres": centres, "dtype": dtype}
        host, metas = self.comm.rendezvous(("regrid_state", tuple(names), grid.nlon, grid.nlat), payload, last)
        if not root:
            return None
        _launch.wait_for(self.device)
        flat = host.numpy()
        out = {"time": windows["time"]} if "time" in windows else {}
        offset = 0
        for m in metas:
            size = _size(m.extent)
            out[m.name] = Quantity(flat[offset:offset + size].reshape(m.extent), m.dims, m.units, origin=(0,) * len(m.dims), extent=m.extent)
            offset += size
        return out

    # ---- scatter -----------------------------------------------------------------------------------------------
    def _gs_global_meta(self, name, q):
        if tuple(q.dims[:1]) != (c.TILE_DIM,):
            raise ValueError(f"scatter sends what gather returns: dims (TILE_DIM, ...), not {q.dims}")
        dtype = q.data.dtype if torch.is_tensor(q.data) else _TORCH_OF[np.dtype(q.data.dtype)]
        return Meta(name, tuple(q.dims[1:]), tuple(q.extent[1:]), q.units, dtype)

    def _gs_global_array(self, q):
        sl = tuple(slice(o, o + e) for o, e in zip(q.origin, q.extent))
        return q.data[sl]

    def _gs_scatter(self, send, recv, tag):
        """send: {name: global Quantity} on the root (None elsewhere); recv: {name: this rank's Quantity} for the names that
        have one.  Returns (metas, {name: received Quantity})."""
        ranks = self.comm.Get_size()
        root = self.rank == c.ROOT_RANK
        mode = self._gs_mode()
        metas = [self._gs_global_meta(n, q) for n, q in send.items()] if (root or mode == "null") and send is not None else None
        if mode in ("cube", "ranks"):
            metas = self.comm.rendezvous(tag + ("meta",), metas, lambda posts: posts[c.ROOT_RANK])
        elif mode == "dist":
            metas = self._gs_bcast([m._replace(dtype=str(m.dtype)) for m in metas] if root else None)
            metas = [m._replace(dtype=getattr(torch, m.dtype.split(".")[-1])) for m in metas]
        elif metas is None:  # a rank without peers and without data: it receives the fill value into what it was given
            for q in recv.values():
                self._gs_global_fill(q)
            return [], dict(recv)
        if not metas:
            return metas, {}
        real = _launch.real_of(self.lib)
        out = {}
        for m in metas:
            if m.name in recv:
                out[m.name] = recv[m.name]
            else:
                out[m.name] = self._gs_factory(m._replace(dtype=real)).empty(m.dims, m.units)
            if tuple(out[m.name].extent) != tuple(m.extent):
                raise ValueError(f"recv_quantity has extent {tuple(out[m.name].extent)}, the scattered tiles {tuple(m.extent)}")
        qs = [out[m.name] for m in metas]
        dtype = metas[0].dtype
        rank_major = mode == "dist"
        layout = _Layout(metas, ranks, rank_major)

        def stage():
            """The root's global arrays as ONE dense device buffer (a single device tensor of the right type is taken as it is)."""
            arrays = [self._gs_global_array(send[m.name]) for m in metas]
            one = arrays[0]
            if (len(arrays) == 1 and torch.is_tensor(one) and one.is_contiguous() and one.device == self.device
                    and one.dtype in (torch.float64, torch.float32)):
                return one.reshape(-1)
            dev, host = self._gs_buffer(layout.total, dtype)
            flat = host.numpy()
            for f, a in enumerate(arrays):
                view = layout.array(flat, f)
                if torch.is_tensor(a):
                    torch.from_numpy(view).copy_(a) if view.flags.c_contiguous else np.copyto(view, a.cpu().numpy())
                else:
                    np.copyto(view, a, casting="same_kind")
            _launch.to_device(host, dev)
            return dev

        if mode in ("cube", "ranks"):
            fused = mode == "cube"

            def last(posts):
                if len({p["stream"] for p in posts.values()}) != 1:
                    raise RuntimeError("the tiles of a gather or scatter called it on different streams: the launch is ordered behind one")
                dense = posts[c.ROOT_RANK]["stage"]()
                if fused:
                    posts[c.ROOT_RANK]["owner"]._gs_launch(True, {r: p["qs"] for r, p in posts.items()}, layout, dense)
                return dense

            dense = self.comm.rendezvous(tag, {"qs": qs, "stream": self._gs_stream_id(), "owner": self, "stage": stage if root else None},
                                         last)
            if not fused:
                self._gs_launch(True, {self.rank: qs}, layout, dense)
                self.comm.barrier()  # the root's buffer lives until every rank has launched
        elif mode == "dist":
            local = torch.empty(layout.per_rank, dtype=dtype, device=self.device)
            dense = stage() if root else None
            _launch.wait_for(self.device)
            self.comm._dist.scatter(local, list(dense.reshape(ranks, -1).unbind(0)) if root else None, src=c.ROOT_RANK,
                                    group=self.comm._group)
            self._gs_launch(True, {self.rank: qs}, layout, local)
        else:
            self._gs_launch(True, {self.rank: qs}, layout, stage())
        return metas, out

    def _gs_global_fill(self, q):
        sl = tuple(slice(o, o + e) for o, e in zip(q.origin, q.extent))
        q.data[sl] = getattr(self.comm, "_fill_value", 0.0)

    def scatter(self, send_quantity=None, recv_quantity=None):
        """communicator.py:111-166: tile r of the root's (TILE_DIM, ...) quantity -- what gather returns -- into the compute
        domain of rank r's ``recv_quantity``, which the communicator's quantity factory allocates when it is absent.  Returns
        recv_quantity."""
        if self.rank == c.ROOT_RANK and send_quantity is None:
            raise TypeError("send_quantity is a required argument on the root rank")
        send = {None: send_quantity} if send_quantity is not None and (self.rank == c.ROOT_RANK or self._gs_mode() == "null") else None
        recv = {None: recv_quantity} if recv_quantity is not None else {}
        _, out = self._gs_scatter(send, recv, ("scatter",))
        return out[None]

    def scatter_state(self, send_state=None, recv_state=None):
        """communicator.py:283-329: every variable of the root's state of global quantities with one launch (and, for host
        arrays, one transfer); ``time`` is handed to every rank."""
        root = self.rank == c.ROOT_RANK
        if root and send_state is None:
            raise TypeError("send_state is a required argument on the root rank")
        if recv_state is None:
            recv_state = {}
        mode = self._gs_mode()
        time = send_state.get("time", None) if send_state is not None else None
        if mode in ("cube", "ranks"):
            time = self.comm.rendezvous(("scatter_state", "time"), time, lambda posts: posts[c.ROOT_RANK])
        elif mode == "dist":
            time = self._gs_bcast(time)
        send = {n: q for n, q in send_state.items() if n != "time"} if send_state is not None and (root or mode == "null") else None
        _, out = self._gs_scatter(send, {n: q for n, q in recv_state.items() if n != "time"}, ("scatter_state",))
        recv_state.update(out)
        if time is not None:
            recv_state["time"] = time
        return recv_state
