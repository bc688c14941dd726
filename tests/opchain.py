"""Per-operator parity of the acoustic loop body on ONE tile at any size.

The oracle walks a synthetic tile through the loop body of AcousticDynamics (dyn_core.py:720-945; single tile: the halo
exchanges are skipped, the halos keep the values of the synthetic state, which is defined on the whole storage).  At every
operator boundary the state before and after the oracle's operator is handed out; the test then runs the PRODUCT operator
(host class -> C ABI -> kernels) on a copy of the same "before" state and compares what the operator writes, on the window
and at the tolerance of the reference's Translate test for that operator:

    D2A2C_Vect 2e-10 (translate_d2a2c_vect.py:47) . C_SW 2e-10 (translate_c_sw.py:107) . UpdateDzC 1e-14 .
    Riem_Solver_C 5e-14 (translate_riem_solver_c.py:33) . PGradC 1e-14 . D_SW 3.2e-10 . UpdateDzD 1e-14 .
    Riem_Solver3 5e-6 (overrides/standard.yaml:49-61) . PE_Halo / PK3_Halo 1e-14 . NH_P_Grad 5e-10 (translate_nh_p_grad.py:8) .
    Ray_Fast 1e-14 . Del2Cubed 1e-14 . apply_diffusive_heating (inside DynCore, 2e-6; held to 1e-13 here)

Operators that contain exp / log / pow (riem_solver_c, riem_solver3, pk3_halo, ray_fast's host table, the heating) can differ
from numpy in the last place on the device; their bounds below say so.
"""
import numpy as np

from helpers import DSW_ARGS, DSW_CFG, compare

from oracle import acoustic_parts as ap
from oracle import cgrid_sw, dgrid_sw, vertical
from oracle import constants as oc
from oracle._np import Grid

P_FAC, RF_CUTOFF, TAU, DELT_MAX, HORD_TM = 0.05, 3000.0, 10.0, 0.002, 6

# ----------------------------------------------------------------------------------------------------------------------
# float32 STORAGE (the _f32 libraries: fields, metrics and K-tables held as float, arithmetic in double).  The oracle stays
# float64; with storage="f32" everything a kernel would LOAD is a float32 value (as float64), so that `before` is exactly what
# ProductOps._load puts into float32 fields and `after` is float32(oracle(before)) -- tests/test_f32_operators.py.
# ----------------------------------------------------------------------------------------------------------------------
F32_MAX = float(np.finfo(np.float32).max)


def f32(a):
    """float64 -> float32 -> float64, clipped to the largest finite float32 first (pk3's 1e40 fill becomes that value, as
    pace_amd/fv3core/stencils/dyn_core.py:135 says); NaN stays NaN."""
    return np.clip(np.asarray(a, dtype=np.float64), -F32_MAX, F32_MAX).astype(np.float32).astype(np.float64)


def f32_dict(d):
    """The float arrays of a dictionary rounded with f32; scalars (dt, ptop, da_min: passed to the kernels as double) untouched."""
    return {k: (f32(v) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in d.items()}


def f32_neighbours(a, rng):
    """Every non-zero finite float32 value of `a` moved to its float32 neighbour, up or down at random (the fill value F32_MAX
    stays): one rounding's worth of storage noise."""
    a32 = np.asarray(a).astype(np.float32)
    up = rng.integers(0, 2, a32.shape).astype(bool)
    with np.errstate(over="ignore"):  # (the neighbour above F32_MAX: not taken)
        moved = np.where(up, np.nextafter(a32, np.float32(np.inf)), np.nextafter(a32, np.float32(-np.inf)))
    keep = (a32 == 0) | ~np.isfinite(a32) | (np.abs(a32) >= np.float32(F32_MAX))
    return np.where(keep, a32, moved).astype(np.float64)


def _win(n, lo=0, hi=0, di=0, dj=0):
    """(i, j) slices: the compute domain widened by lo cells below / hi above, + di / dj staggered points."""
    return (slice(3 - lo, 3 + n + hi + di), slice(3 - lo, 3 + n + hi + dj))


class OpCase:
    """name, state before, state after (oracle), checks = [(variable, (i, j) window, number of levels, tolerance, near_zero
    as a fraction of the field's magnitude)]."""

    def __init__(self, name, before, after, checks):
        self.name, self.before, self.after, self.checks = name, before, after, checks


def column(nz):
    from pace_amd.fv3core import DGridShallowWaterLagrangianDynamicsConfig
    from pace_amd.fv3core.stencils.d_sw import column_namelist_arrays

    return column_namelist_arrays(DGridShallowWaterLagrangianDynamicsConfig(**DSW_CFG), nz)


class Chain:
    def __init__(self, n, nz, metrics=None, state=None, storage=None):
        """storage=None: the float64 chain.  storage="f32": metrics (before Grid is built), column tables, the initial state and
        the whole state at every operator boundary are float32 values (f32 above); the arithmetic stays float64."""
        from pace_amd import synthetic

        assert storage in (None, "f32")
        self.n, self.nz, self.storage = n, nz, storage
        self.metrics = metrics if metrics is not None else synthetic.tile_metrics(n, nz)
        s = state if state is not None else synthetic.acoustic_state(self.metrics, n, nz)
        self.col = column(nz)
        if storage:
            self.metrics, s, self.col = f32_dict(self.metrics), f32_dict(s), f32_dict(self.col)
        self.g = Grid(n, nz, self.metrics)
        self.dt = float(s["dt"])
        self.ptop = float(self.metrics["ptop"])
        z3 = lambda: np.zeros(s["u"].shape)  # noqa: E731
        S = {k: s[k].copy() for k in ("delp", "pt", "u", "v", "w", "uc", "vc", "ua", "va", "q_con", "cappa", "delz", "pe", "pk", "peln")}
        S.update(zs=s["zs"].copy(), phis=s["zs"] * oc.GRAV, ws3=np.zeros(s["zs"].shape), wsd=np.zeros(s["zs"].shape))
        for k in ("ut", "vt", "divgd", "omga", "delpc", "ptc", "pkc", "mfxd", "mfyd", "cxd", "cyd", "crx", "cry", "xfx", "yfx",
                  "heat_source", "diss_estd", "utc", "vtc"):
            S[k] = z3()
        S["zh"] = s["zh"].copy()
        S["gz"] = s["zh"].copy()  # dyn_core.py:760-776: on the first substep zh := gz (heights, like the reference's gz here)
        S["pk3"] = np.full(s["u"].shape, 1.0e40)
        self.S = S
        self._store()
        self.csw = cgrid_sw.CSWState(s["u"].shape)
        self.dsw = dgrid_sw.DSWState(s["u"].shape)

    def _snap(self):
        return {k: v.copy() for k, v in self.S.items()}

    def _store(self):
        """An operator boundary: with float32 storage the whole state goes through `real` fields."""
        if self.storage:
            for v in self.S.values():
                v[...] = f32(v)

    def cases(self, only=None, inject=None):
        """Generator of OpCase in loop order.  The chain always advances through every operator (later ones need the
        fields of the earlier ones); ``only`` just limits what is handed out.  ``inject(name)``, if given, returns the state
        that replaces this chain's own before operator `name` (the noise pass of tests/test_f32_operators.py: a second chain
        fed the perturbed `before` of the first).  With float32 storage every case carries `raw`: the oracle's checked
        outputs BEFORE they are rounded for storage."""
        S, g, n, nz = self.S, self.g, self.n, self.nz
        dt, dt2, ptop = self.dt, 0.5 * self.dt, self.ptop
        K = nz + 1
        C0, C1 = _win(n), _win(n, 1, 1)

        def take(name):
            if inject is not None:
                for k, v in inject(name).items():
                    S[k][...] = v

        def emit(name, fn, checks):
            want = only is None or name in only
            take(name)
            before = self._snap() if want else None
            fn()
            raw = {c[0]: S[c[0]].copy() for c in checks} if want and self.storage else None
            self._store()
            if want:
                case = OpCase(name, before, self._snap(), checks)
                case.raw = raw
                yield case

        # --- D2A2C_Vect on the initial winds (translate_d2a2c_vect.py:36-47); does not advance the chain ---
        if only is None or "d2a2c_vect" in only:
            saved = self._snap() if inject is not None else None
            take("d2a2c_vect")
            before = self._snap()
            T = {k: S[k].copy() for k in ("uc", "vc", "u", "v", "ua", "va", "utc", "vtc")}
            cgrid_sw.d2a2c_vect(g, cgrid_sw.D2A2CState(S["u"].shape), T["uc"], T["vc"], T["u"], T["v"], T["ua"], T["va"], T["utc"], T["vtc"])
            after = dict(before)
            after.update(T)
            W1 = _win(n, 1, 1)
            case = OpCase("d2a2c_vect", before, after,
                          [("uc", _win(n, 1, 1, 1, 0), nz, 2e-10, 1e-13), ("vc", _win(n, 1, 1, 0, 1), nz, 2e-10, 1e-13),
                           ("ua", W1, nz, 2e-10, 1e-13), ("va", W1, nz, 2e-10, 1e-13),
                           ("utc", _win(n, 1, 1, 1, 0), nz, 2e-10, 1e-13), ("vtc", _win(n, 1, 1, 0, 1), nz, 2e-10, 1e-13)])
            case.raw = None
            if self.storage:
                case.raw = {c[0]: T[c[0]] for c in case.checks}
                case.after = f32_dict(after)
            if saved is not None:  # (this operator does not advance the chain: neither does what was injected for it)
                for k, v in saved.items():
                    S[k][...] = v
            yield case

        def f_csw():
            cgrid_sw.c_sw(g, self.csw, S["delp"], S["pt"], S["u"], S["v"], S["w"], S["uc"], S["vc"], S["ua"], S["va"], S["ut"], S["vt"],
                          S["divgd"], S["omga"], dt2, nord=DSW_CFG["nord"])
            S["delpc"][...] = self.csw.delpc
            S["ptc"][...] = self.csw.ptc

        # translate_c_sw.py:85-107: delpc, ptc, omga on compute +- 1, uc / vc on their staggered compute windows, divgd on corners
        yield from emit("c_sw", f_csw, [("delpc", C1, nz, 2e-10, 0), ("ptc", C1, nz, 2e-10, 0), ("omga", C1, nz, 2e-10, 1e-12),
                                        ("uc", _win(n, 0, 0, 1, 0), nz, 2e-10, 1e-12), ("vc", _win(n, 0, 0, 0, 1), nz, 2e-10, 1e-12),
                                        ("ua", C1, nz, 2e-10, 1e-12), ("va", C1, nz, 2e-10, 1e-12),
                                        ("ut", C1, nz, 2e-10, 1e-12), ("vt", C1, nz, 2e-10, 1e-12),
                                        ("divgd", _win(n, 0, 0, 1, 1), nz, 2e-10, 1e-10)])

        def f_dzc():
            S["zh"][:-1, :-1, :] = S["gz"][:-1, :-1, :]
            vertical.update_dz_c(g, g.dp_ref, S["zs"], S["ut"], S["vt"], S["gz"], S["ws3"], dt2)

        yield from emit("updatedzc", f_dzc, [("gz", C1, K, 1e-14, 0), ("ws3", C1, None, 1e-14, 1e-12)])

        def f_riemc():
            vertical.riem_solver_c(g, dt2, S["cappa"], ptop, S["phis"], S["ws3"], S["ptc"], S["q_con"], S["delpc"], S["gz"], S["pkc"],
                                   S["omga"], p_fac=P_FAC)

        # the reference's own bound: 5e-14 (translate_riem_solver_c.py:33); measured on MI355X: 1.5e-15
        yield from emit("riem_solver_c", f_riemc, [("pkc", C1, K, 5e-14, 0), ("gz", C1, K, 5e-14, 0)])

        yield from emit("p_grad_c", lambda: ap.p_grad_c(g, S["uc"], S["vc"], S["delpc"], S["pkc"], S["gz"], dt2),
                        [("uc", _win(n, 0, 0, 1, 0), nz, 1e-13, 1e-12), ("vc", _win(n, 0, 0, 0, 1), nz, 1e-13, 1e-12)])

        def f_dsw():
            dgrid_sw.d_sw(g, self.col, DSW_CFG, self.dsw, S["vt"], S["delp"], S["pt"], S["u"], S["v"], S["w"], S["uc"], S["vc"], S["ua"],
                          S["va"], S["divgd"], S["mfxd"], S["mfyd"], S["cxd"], S["cyd"], S["crx"], S["cry"], S["xfx"], S["yfx"], S["q_con"],
                          S["zh"], S["heat_source"], S["diss_estd"], dt)

        dchecks = []
        # translate_d_sw.py:36-65: every argument but zh, incl. what is left in the work fields uc, vc, divgd and delpc (= vt here)
        for k in ("delp", "pt", "u", "v", "w", "q_con", "mfxd", "mfyd", "cxd", "cyd", "crx", "cry", "xfx", "yfx", "heat_source", "diss_estd",
                  "uc", "vc", "divgd", "vt"):
            di = 1 if k in ("mfxd", "cxd", "crx", "xfx", "v", "uc", "divgd", "vt") else 0
            dj = 1 if k in ("mfyd", "cyd", "cry", "yfx", "u", "vc", "divgd", "vt") else 0
            dchecks.append((k, _win(n, 0, 0, di, dj), nz, 3.2e-10, 1e-12))
        yield from emit("d_sw", f_dsw, dchecks)

        def f_dzd():
            vertical.update_dz_d(g, self.col, g.dp_ref, S["zs"], S["zh"], S["crx"], S["cry"], S["xfx"], S["yfx"], S["wsd"], dt,
                                 hord_tm=HORD_TM)

        yield from emit("updatedzd", f_dzd, [("zh", C0, K, 1e-14, 0), ("wsd", C0, None, 1e-14, 1e-12)])

        def f_riem3():
            vertical.riem_solver3(g, True, dt, S["cappa"], ptop, S["zs"], S["wsd"], S["delz"], S["q_con"], S["delp"], S["pt"], S["zh"],
                                  S["pe"], S["pkc"], S["pk3"], S["pk"], S["peln"], S["w"], p_fac=P_FAC)

        yield from emit("riem_solver3", f_riem3, [("delz", C0, nz, 5e-6, 0), ("zh", C0, K, 5e-6, 0), ("pkc", C0, K, 5e-6, 1e-5),
                                                  ("pk3", C0, K, 5e-6, 0), ("w", C0, nz, 5e-6, 1e-5), ("pe", C0, K, 5e-6, 0),
                                                  ("pk", C0, K, 5e-6, 0), ("peln", C0, K, 5e-6, 0)])

        yield from emit("edge_pe", lambda: ap.edge_pe(g, S["pe"], S["delp"], ptop), [("pe", C1, K, 1e-14, 0)])
        # pow on the device vs numpy: last-place differences
        yield from emit("pk3_halo", lambda: ap.pk3_halo(g, S["pk3"], S["delp"], ptop, oc.KAPPA), [("pk3", _win(n, 2, 2), K, 1e-14, 0)])

        def f_geo():
            S["gz"][1:-2, 1:-2, :] = S["zh"][1:-2, 1:-2, :] * oc.GRAV

        yield from emit("compute_geopotential", f_geo, [("gz", _win(n, 2, 2), K, 0.0, 0)])

        yield from emit("nh_p_grad", lambda: ap.nh_p_grad(g, S["u"], S["v"], S["pkc"], S["gz"], S["pk3"], S["delp"], dt, ptop, oc.KAPPA),
                        [("u", _win(n, 0, 0, 0, 1), nz, 5e-10, 1e-12), ("v", _win(n, 0, 0, 1, 0), nz, 5e-10, 1e-12),
                         ("pkc", _win(n, 0, 0, 1, 1), K, 5e-10, 1e-9), ("gz", _win(n, 0, 0, 1, 1), K, 5e-10, 0),
                         ("pk3", _win(n, 0, 0, 1, 1), K, 5e-10, 0)])

        yield from emit("ray_fast", lambda: ap.ray_fast(g, S["u"], S["v"], S["w"], g.dp_ref, g.p, dt, ptop, rf_cutoff=RF_CUTOFF, tau=TAU),
                        [("u", _win(n, 0, 0, 0, 1), nz, 1e-13, 1e-12), ("v", _win(n, 0, 0, 1, 0), nz, 1e-13, 1e-12),
                         ("w", C0, nz, 1e-13, 1e-12)])

        yield from emit("del2cubed", lambda: ap.del2_cubed(g, S["heat_source"], oc.CNST_0P20 * g.da_min, 3),
                        [("heat_source", C0, nz, 1e-14, 1e-12)])

        yield from emit("apply_diffusive_heating",
                        lambda: ap.apply_diffusive_heating(g, S["delp"], S["delz"], S["cappa"], S["heat_source"], S["pt"],
                                                           abs(dt * DELT_MAX), nz),
                        [("pt", C0, nz, 1e-13, 0)])


class ProductOps:
    """The host classes of one tile, built once; run(name, before) applies one operator to a state given as numpy arrays and
    returns the numpy arrays afterwards."""

    def __init__(self, lib, device, chain):
        from helpers import Env
        from pace_amd.fv3core import DGridShallowWaterLagrangianDynamicsConfig, RiemannConfig
        from pace_amd.fv3core.stencils.c_sw import CGridShallowWaterDynamics
        from pace_amd.fv3core.stencils.d2a2c_vect import DGrid2AGrid2CGridVectors
        from pace_amd.fv3core.stencils.d_sw import DGridShallowWaterLagrangianDynamics
        from pace_amd.fv3core.stencils.del2cubed import HyperdiffusionDamping
        from pace_amd.fv3core.stencils.nh_p_grad import NonHydrostaticPressureGradient
        from pace_amd.fv3core.stencils.pk3_halo import PK3Halo
        from pace_amd.fv3core.stencils.ray_fast import RayleighDamping
        from pace_amd.fv3core.stencils.riem_solver3 import NonhydrostaticVerticalSolver
        from pace_amd.fv3core.stencils.riem_solver_c import NonhydrostaticVerticalSolverCGrid
        from pace_amd.fv3core.stencils.updatedzc import UpdateGeopotentialHeightOnCGrid
        from pace_amd.fv3core.stencils.updatedzd import UpdateHeightOnDGrid

        n, nz = chain.n, chain.nz
        self.chain, self.lib = chain, lib
        self.env = env = Env(lib, device, chain.metrics, n, nz)
        sf, qf, gd, dc = env.stencil_factory, env.qf, env.grid_data, env.damping
        colq = {k: env.kq(v) for k, v in chain.col.items()}
        self.d2a2c = DGrid2AGrid2CGridVectors(sf, qf, gd, False, 0, True)
        self.csw = CGridShallowWaterDynamics(sf, qf, gd, False, 0, DSW_CFG["nord"])
        self.dzc = UpdateGeopotentialHeightOnCGrid(sf, qf, gd.area, gd.dp_ref, grid_data=gd)
        self.riemc = NonhydrostaticVerticalSolverCGrid(sf, qf, P_FAC)
        self.dsw = DGridShallowWaterLagrangianDynamics(sf, qf, gd, dc, colq, False, False, DGridShallowWaterLagrangianDynamicsConfig(**DSW_CFG))
        self.dzd = UpdateHeightOnDGrid(sf, qf, dc, gd, 0, HORD_TM, colq)
        self.riem3 = NonhydrostaticVerticalSolver(sf, qf, RiemannConfig(p_fac=P_FAC))
        self.nh = NonHydrostaticPressureGradient(sf, qf, gd, 0)
        self.pk3h = PK3Halo(sf, qf)
        self.ray = RayleighDamping(sf, RF_CUTOFF, TAU, False, quantity_factory=qf)
        self.del2 = HyperdiffusionDamping(sf, qf, dc, gd.rarea, 3)
        self.fields = {}

    def _load(self, before):
        env = self.env
        for k, a in before.items():
            if k not in self.fields:
                self.fields[k] = env.q2() if a.ndim == 2 else env.q3()
            self.fields[k].set(a)
        return self.fields

    def run(self, name, before):
        import ctypes as C

        import torch

        from pace_amd.fv3core.stencils._common import dptr

        f = self._load(before)
        ch = self.chain
        dt, dt2, ptop = ch.dt, 0.5 * ch.dt, ch.ptop
        geom, met, st = self.csw._geom, self.csw._met, self.csw.stream

        def call(fn, *a):
            self.lib.call(fn, C.byref(geom), *a)

        if name == "d2a2c_vect":
            self.d2a2c(f["uc"], f["vc"], f["u"], f["v"], f["ua"], f["va"], f["utc"], f["vtc"])
        elif name == "c_sw":
            self.csw(f["delp"], f["pt"], f["u"], f["v"], f["w"], f["uc"], f["vc"], f["ua"], f["va"], f["ut"], f["vt"], f["divgd"], f["omga"], dt2)
            f["delpc"].data[...] = self.csw.delpc.data
            f["ptc"].data[...] = self.csw.ptc.data
        elif name == "updatedzc":
            call("pace_copy", dptr(f["gz"]), dptr(f["zh"]), st())
            self.dzc(f["zs"], f["ut"], f["vt"], f["gz"], f["ws3"], dt2)
        elif name == "riem_solver_c":
            self.riemc(dt2, f["cappa"], ptop, f["phis"], f["ws3"], f["ptc"], f["q_con"], f["delpc"], f["gz"], f["pkc"], f["omga"])
        elif name == "p_grad_c":
            call("pace_p_grad_c", C.byref(met), dptr(f["uc"]), dptr(f["vc"]), dptr(f["delpc"]), dptr(f["pkc"]), dptr(f["gz"]), dt2, st())
        elif name == "d_sw":
            names = dict(delpc="vt", mfx="mfxd", mfy="mfyd", cx="cxd", cy="cyd", diss_est="diss_estd")
            # uc_contra / vc_contra of the previous call are the head of the workspace: the oracle's DSWState starts at zero
            self.dsw._workspace[: 2 * f["u"]._base.numel()] = 0.0
            self.dsw(*[f[names.get(k, k)] for k in DSW_ARGS], dt)
        elif name == "updatedzd":
            self.dzd(f["zs"], f["zh"], f["crx"], f["cry"], f["xfx"], f["yfx"], f["wsd"], dt)
        elif name == "riem_solver3":
            self.riem3(True, dt, f["cappa"], ptop, f["zs"], f["wsd"], f["delz"], f["q_con"], f["delp"], f["pt"], f["zh"], f["pe"], f["pkc"],
                       f["pk3"], f["pk"], f["peln"], f["w"])
        elif name == "edge_pe":
            call("pace_edge_pe", dptr(f["pe"]), dptr(f["delp"]), ptop, st())
        elif name == "pk3_halo":
            self.pk3h(f["pk3"], f["delp"], ptop, oc.KAPPA)
        elif name == "compute_geopotential":
            call("pace_compute_geopotential", dptr(f["zh"]), dptr(f["gz"]), st())
        elif name == "nh_p_grad":
            self.nh(f["u"], f["v"], f["pkc"], f["gz"], f["pk3"], f["delp"], dt, ptop, oc.KAPPA)
        elif name == "ray_fast":
            self.ray(f["u"], f["v"], f["w"], self.env.grid_data.dp_ref, self.env.grid_data.p, dt, ptop)
        elif name == "del2cubed":
            self.del2(f["heat_source"], oc.CNST_0P20 * self.env.damping.da_min)
        elif name == "apply_diffusive_heating":
            call("pace_apply_diffusive_heating", dptr(f["delp"]), dptr(f["delz"]), dptr(f["cappa"]), dptr(f["heat_source"]), dptr(f["pt"]),
                 abs(dt * DELT_MAX), ch.nz, st())
        else:
            raise KeyError(name)
        if self.env.qf.device.type == "cuda":
            torch.cuda.synchronize()
        return f


# On a BALANCED state (the baroclinic case on the sphere) the C-grid solver's perturbation pressure pkc is (full pressure -
# hydrostatic pressure), 1e-4 ... 1e-3 of either, and both come out of exp / log whose last place differs between the device
# and numpy: 1e-16 of the pressure is 1e-12 of the perturbation (measured on MI355X: 1.1e-12 of max |pkc| at C48 and C96; the
# synthetic state, whose perturbation is as large as the pressure, gives 1.5e-15).  The height gz it returns inherits the same
# through the dz update.  (operator, variable) -> (tolerance of the relative metric, floor as a fraction of the magnitude,
# bound on max |error| / magnitude or None where the window holds fill values).  Every operator WITHOUT a transcendental is
# held to an absolute error of 1e-14 of the magnitude on the sphere as well (measured: exactly 0).
SPHERE_CHECKS = {("riem_solver_c", "pkc"): (1e-9, 1e-2, 1e-11), ("riem_solver_c", "gz"): (1e-11, 0.0, None)}
# the operators of the single-tile chain that make sense on a captured sphere state: the chain has no halo exchanges (the
# synthetic state is defined on the whole storage; a captured tile's halos are those of ONE instant of the loop), so from the
# D-grid vertical solver on the chain runs on inconsistent halo columns.  riem_solver3 on the sphere: the full-field test of
# tests/test_gpu_sphere.py; the operators after it: the six-tile loop with its exchanges (geometry "sphere").
SPHERE_CHAIN = ("d2a2c_vect", "c_sw", "updatedzc", "riem_solver_c", "p_grad_c", "d_sw", "updatedzd")


# Outputs an operator only WRITES (it never reads what they held): with poison=True check_case fills their checked windows with
# NaN before the call, as the chain fills pk3 with 1e40 -- a workgroup that is skipped then leaves NaN where the oracle has a
# number.  (An entry that the operator did read would fail at once, under emulation as on the device: NaN propagates.)
WRITE_ONLY = {
    "d2a2c_vect": ("uc", "vc", "ua", "va", "utc", "vtc"),
    "c_sw": ("omga", "uc", "vc", "ua", "va", "ut", "vt", "divgd"),
    "updatedzc": ("ws3",),
    "riem_solver_c": ("pkc",),
    "d_sw": ("crx", "cry", "xfx", "yfx", "diss_estd", "vt"),
    "updatedzd": ("wsd",),
    "riem_solver3": ("delz", "pkc", "pk3", "pe", "pk", "peln"),
    "compute_geopotential": ("gz",),
}


def poisoned(case):
    """case.before with NaN in the checked windows of the outputs the operator only writes."""
    before = dict(case.before)
    for var, win, nk, _, _ in case.checks:
        if var in WRITE_ONLY.get(case.name, ()):
            a = before[var] = before[var].copy()
            if a.ndim == 3:
                a[win + (slice(0, nk),)] = np.nan
            else:
                a[win] = np.nan
    return before


def check_case(ops, case, scale_tol=1.0, report=None, sphere=False, poison=False):
    """Run the product operator on case.before and compare with case.after.  Returns {variable: error}."""
    f = ops.run(case.name, poisoned(case) if poison else case.before)
    errs = {}
    bad = []
    for var, win, nk, tol, nz_frac in case.checks:
        ref = case.after[var]
        got = f[var].numpy()
        if ref.ndim == 3:
            r, gt = ref[win][:, :, :nk], got[win][:, :, :nk]
        else:
            r, gt = ref[win], got[win]
        assert np.isfinite(r).all(), (case.name, var, "oracle produced non-finite values")
        scale = float(np.abs(r).max())
        abs_tol = max(tol, 1e-14)
        if sphere and (case.name, var) in SPHERE_CHECKS:
            tol, nz_frac, abs_tol = SPHERE_CHECKS[(case.name, var)]
        near = nz_frac * scale if nz_frac else 0.0
        e = compare(r, gt, near_zero=near)
        errs[var] = e
        ab = float(np.abs(r - gt).max()) / (scale + 1e-300)
        if report is not None:
            report.setdefault(case.name, {})[var] = e
            report[case.name][var + ".metric_no_floor"] = compare(r, gt)
            report[case.name][var + ".abs_over_magnitude"] = ab
        if not e <= tol * scale_tol:
            bad.append((case.name, var, e, tol))
        if sphere and abs_tol is not None and not ab <= abs_tol * scale_tol:  # the absolute error, everywhere
            bad.append((case.name, var, "abs/magnitude", ab, abs_tol))
    assert not bad, bad
    return errs


# ----------------------------------------------------------------------------------------------------------------------
# The whole AcousticDynamics call on six synthetic tiles of any size (every operator chained on its predecessor's output,
# all halo-update groups), product against oracle/dyn_core.py
# ----------------------------------------------------------------------------------------------------------------------
LOOP_STATE = "u v w delz delp pt pe pk peln phis uc vc ua va q_con".split()
LOOP_OUT = "u v w delz delp pt pe pk peln q_con omga ua va uc vc mfxd mfyd cxd cyd diss_estd heat_source".split()


def six_tile_inputs(n, nz):
    """Six copies of the synthetic tile, each with its own amplitude of the wave / vertical-velocity perturbation, joined by the
    cubed-sphere halo exchange (the geometry is the same single tile for all six: a consistency configuration, not a sphere)."""
    from pace_amd import synthetic

    m = synthetic.tile_metrics(n, nz)
    tiles = []
    for t in range(6):
        s = synthetic.acoustic_state(m, n, nz)
        a = {k: s[k].copy() for k in LOOP_STATE if k != "phis"}
        a["phis"] = s["zs"] * oc.GRAV
        a["w"] *= 1.0 + 0.3 * t
        a["pt"][:, :, :nz] *= 1.0 + 1.0e-3 * t
        a["v"] *= 1.0 - 0.05 * t
        tiles.append((a, s["cappa"].copy()))
    return m, tiles


def six_tile_inputs_sphere(n, nz):
    """The six tiles of the gnomonic cubed sphere (pace_amd.util.gridgen: edge-averaged metrics, six distinct tiles) with the
    Jablonowski-Williamson state of the baroclinic case (halos as the initialisation leaves them: the loop's own exchanges fill
    them), plus a smooth vertical-velocity perturbation and a small condensate loading so that every term of the loop is
    exercised.  Returns ([metrics per tile], [(arrays, cappa) per tile])."""
    from pace_amd.fv3core.initialization.baroclinic import baroclinic_state_six_tiles
    from pace_amd.util import gridgen

    grid = gridgen.tiles(n, nz)
    states = baroclinic_state_six_tiles(grid, n, nz)
    metrics, tiles = [], []
    kk = np.arange(nz + 1)[None, None, :]
    for t in range(6):
        g = {k: v for k, v in grid[t].items() if k not in ("ee1", "ee2", "es1", "ew2")}
        st = states[t]
        a = {k: np.array(st[k], dtype=np.float64) for k in LOOP_STATE}
        lon, lat = g["lon_agrid"], g["lat_agrid"]
        c = (slice(3, 3 + n), slice(3, 3 + n))
        a["w"][c] = (0.3 * np.sin(3.0 * lon[c]) * np.cos(lat[c]))[:, :, None] * np.sin(np.pi * kk / nz)
        a["q_con"] = np.zeros_like(a["pt"])
        a["q_con"][c] = (1.0e-4 * (1.0 + np.cos(2.0 * lon[c]) * np.cos(lat[c])))[:, :, None] * (kk / nz) ** 2
        cappa = np.full(a["pt"].shape, oc.KAPPA)
        metrics.append(g)
        tiles.append((a, cappa))
    return metrics, tiles


def loop_inputs(n, nz, geometry):
    """([metrics per tile], [(arrays, cappa) per tile]) for geometry "synthetic" (six copies of one tile) or "sphere"."""
    if geometry == "sphere":
        return six_tile_inputs_sphere(n, nz)
    m, tiles = six_tile_inputs(n, nz)
    return [m] * 6, tiles


def oracle_loop(n, nz, n_split, timestep, geometry="synthetic"):
    from oracle import dyn_core

    ms, tiles = loop_inputs(n, nz, geometry)
    grids = [Grid(n, nz, ms[t]) for t in range(6)]
    states = []
    for a, _ in tiles:
        st = {k: v.copy() for k, v in a.items()}
        for k in ("omga", "mfxd", "mfyd", "cxd", "cyd", "diss_estd"):
            st[k] = np.zeros(a["u"].shape)
        states.append(st)
    cappas = [c.copy() for _, c in tiles]
    cfg = dict(DSW_CFG, p_fac=P_FAC, rf_cutoff=RF_CUTOFF, tau=TAU, delt_max=DELT_MAX, hord_tm=HORD_TM)
    tmp = dyn_core.acoustic_dynamics(grids, column(nz), cfg, states, cappas, timestep, n_split, n, nz)
    for t in range(6):
        states[t]["heat_source"] = tmp[t].heat_source
    return states


def product_loop_tile(comm, lib, device, m, arrays, cappa, n, nz, n_split, timestep):
    import torch

    from helpers import Env, acoustic_config
    from pace_amd.fv3core.initialization.dycore_state import DycoreState
    from pace_amd.fv3core.stencils.dyn_core import AcousticDynamics
    from pace_amd.util import CubedSphereCommunicator

    env = Env(lib, device, m, n, nz)
    cube = CubedSphereCommunicator(comm, device=device, lib=lib)
    state = DycoreState.init_from_numpy_arrays(arrays, env.qf)
    dyn = AcousticDynamics(cube, env.stencil_factory, env.qf, env.grid_data, env.damping, 0, False, False, acoustic_config(n_split),
                           state.phis, env.q2(), state)
    dyn.cappa.set(cappa)
    dyn(state, timestep=timestep, n_map=1)
    if env.qf.device.type == "cuda":
        torch.cuda.synchronize()
    out = {k: getattr(state, k).numpy() for k in LOOP_OUT if k != "heat_source"}
    out["heat_source"] = dyn._heat_source.numpy()
    return out


def product_loop(lib, device, n, nz, n_split, timestep, geometry="synthetic"):
    from pace_amd.util import run_tiles

    ms, tiles = loop_inputs(n, nz, geometry)
    return run_tiles(6, lambda comm: product_loop_tile(comm, lib, device, ms[comm.Get_rank()], tiles[comm.Get_rank()][0],
                                                       tiles[comm.Get_rank()][1], n, nz, n_split, timestep))


# The reference's bound for the whole acoustic call is 2e-6 for every variable (translate_dyncore.py:120-121): held here.  Measured on MI355X at C96 x 79 (profiles/r02_acoustic_loop_c96_gpu_errors.json): masses,
# temperatures and pressures agree to 4e-15, winds / mass fluxes / Courant numbers to 1e-7 (last-place differences of the
# device's exp / log in the two vertical solvers, carried through the pressure-gradient and transport steps), w to 3e-6.
LOOP_TOL = {"w": 2e-6, "omga": 2e-6, "delz": 2e-6, "diss_estd": 2e-6, "heat_source": 2e-6,
            "u": 2e-6, "v": 2e-6, "ua": 2e-6, "va": 2e-6, "uc": 2e-6, "vc": 2e-6, "mfxd": 2e-6, "mfyd": 2e-6, "cxd": 2e-6, "cyd": 2e-6,
            "delp": 1e-11, "pt": 1e-11, "pe": 1e-11, "pk": 1e-11, "peln": 1e-11, "q_con": 1e-11}
# (masses, temperatures, pressures: measured 1e-12 at C96, 3e-12 at C192 -- profiles/r06_acoustic_loop_c192_sphere_gpu_errors.json)


# Variables with entries that are residue of cancelling terms (dissipation sums, w / omga and the winds near their zero
# crossings, fluxes across symmetry lines): the reference's relative metric means nothing below this fraction of the field's
# magnitude (the reference's Translate tests carry per-variable near_zero overrides for the same reason,
# tests/savepoint/translate/overrides/standard.yaml).  Everything else -- masses, temperatures, pressures -- gets NO floor.
# (diss_estd / heat_source are built from w -- heat_diss, d_sw.py:63-103 -- and inherit the vertical solver's ABSOLUTE error of
# ~1e-11 of w's magnitude: an entry 1e-5 of the field's largest has a relative error of 1e-6)
LOOP_NEAR_ZERO = {"w": 1e-5, "omga": 1e-5, "diss_estd": 1e-4, "heat_source": 1e-4, "u": 1e-8, "v": 1e-8, "ua": 1e-8, "va": 1e-8,
                  "uc": 1e-8, "vc": 1e-8, "mfxd": 1e-8, "mfyd": 1e-8, "cxd": 1e-8, "cyd": 1e-8}


# On the balanced state of the sphere the pressure-gradient force is a small residual of large terms, so every wind and flux
# carries the vertical solvers' absolute error (~1e-11 of the field's magnitude, measured 4e-11 at C96) also where the zonal-flow
# case leaves it small: the relative metric applies above 1e-4 of the magnitude, and the ABSOLUTE error is bounded everywhere
# (LOOP_ABS_SPHERE, fractions of the magnitude; measured maxima are 10 to 100 times smaller).
LOOP_NEAR_ZERO_SPHERE = dict(LOOP_NEAR_ZERO, **{k: 1e-4 for k in ("u", "v", "ua", "va", "uc", "vc", "mfxd", "mfyd", "cxd", "cyd")})
LOOP_ABS_SPHERE = 1e-9
# ... and on the synthetic tiles too, where the floors above would otherwise hide an error in small entries (measured maxima on
# MI355X at C96: 5e-11 for w, <= 2e-13 for everything else; profiles/r03_acoustic_loop_c96_synthetic_gpu_errors.json)
LOOP_ABS_SYNTHETIC = 1e-10


def loop_errors(ref, got, n, nz, detail=None, geometry="synthetic"):
    """Worst error per variable over the six tiles in the reference's metric, with the per-variable floor of LOOP_NEAR_ZERO.
    `detail` (a dict) receives, per variable, the UNMASKED maxima as well: relative metric without any floor, absolute error,
    absolute error over the field's magnitude -- what profiles/r03_acoustic_loop_c96_gpu_errors.json records."""
    errs = {}
    for k in LOOP_OUT:
        di = 1 if k in ("v", "mfxd", "cxd", "uc") else 0
        dj = 1 if k in ("u", "mfyd", "cyd", "vc") else 0
        nk = nz + 1 if k in ("pe", "pk", "peln") else nz
        W = (slice(3, 3 + n + di), slice(3, 3 + n + dj), slice(0, nk))
        worst, raw, absmax, absrel = 0.0, 0.0, 0.0, 0.0
        for t in range(6):
            r = ref[t][k][W]
            assert np.isfinite(r).all(), (k, t)
            o = got[t][k][W]
            scale = float(np.abs(r).max()) + 1e-300
            floors = LOOP_NEAR_ZERO_SPHERE if geometry == "sphere" else LOOP_NEAR_ZERO
            worst = max(worst, compare(r, o, near_zero=floors.get(k, 0.0) * scale))
            raw = max(raw, compare(r, o))
            absmax = max(absmax, float(np.abs(r - o).max()))
            absrel = max(absrel, float(np.abs(r - o).max()) / scale)
        errs[k] = worst
        if detail is not None:
            detail[k] = {"metric_with_floor": worst, "floor_fraction_of_magnitude": floors.get(k, 0.0), "metric_no_floor": raw,
                         "max_abs_error": absmax, "max_abs_error_over_magnitude": absrel}
    return errs


# ----------------------------------------------------------------------------------------------------------------------
# The operators the reference also tests on their own (TranslateXPPM / YPPM / DivergenceDamping) as stand-alone classes
# ----------------------------------------------------------------------------------------------------------------------
def staged_bound(scale, S, factor=2.0):
    """The bound on max |got - float32(ref)| of an output with intermediates in `real` storage: one float32 ulp of the magnitude
    `scale` = max |ref| for the output's own rounding + factor x the oracle's response S to one rounding of its inputs
    (tests/test_f32_operators.py has the reasoning).  The one place it is written."""
    return 2.0 ** -23 * scale + factor * S


def _staged_f32(name, got, ref, noisy, report):
    """float32 storage, an output with intermediates in `real` storage, against staged_bound with
    S = max |oracle(inputs (+) noise) - oracle(inputs)| over the draws `noisy`."""
    assert got.dtype == np.float32, (name, got.dtype)
    S = max(float(np.abs(x - ref).max()) for x in noisy)
    err = float(np.abs(got.astype(np.float64) - f32(ref)).max())
    scale = float(np.abs(ref).max())
    if report is not None:
        report[name] = dict(err_in_u=err / (2.0 ** -24 * scale + 1e-300), err_over_S=err / S if S > 0 else (0.0 if err == 0 else np.inf))
    assert err <= staged_bound(scale, S), (name, err, scale, S)
    return err / (scale + 1e-300)


def check_standalone_operators(lib, device, n, nz, exact, storage=None, report=None):
    """XPiecewiseParabolic / YPiecewiseParabolic (iord 5, 6, 8; the windows fvtp2d uses: inner = compute x full, outer =
    compute + 1) and DivergenceDamping against the oracle.  Returns {name: error}.

    storage="f32" (a float32-storage library): metrics, column tables and every input are float32 values; XPPM / YPPM (one pass
    from loads to stores) must equal float32(oracle) bit for bit, as must DivergenceDamping's divgd, uc and vc; its vort_b, ke and
    delpc and Sim1Solver's outputs (intermediates in `real` storage) are held to the staged bound of _staged_f32, with the oracle's
    response to storage noise from two draws of f32_neighbours.  `report` then receives {name: error in u = 2^-24 max |ref|, error / S}."""
    import torch

    from helpers import Env
    from oracle import damping
    from oracle import ppm_transport as tr
    from pace_amd import synthetic
    from pace_amd.fv3core.stencils.divergence_damping import DivergenceDamping
    from pace_amd.fv3core.stencils.xppm import XPiecewiseParabolic
    from pace_amd.fv3core.stencils.yppm import YPiecewiseParabolic

    assert storage in (None, "f32") and (storage is None) == (lib.real_bytes == 8)
    m = synthetic.tile_metrics(n, nz)
    s = synthetic.acoustic_state(m, n, nz)
    col = column(nz)
    if storage:
        m, s, col = f32_dict(m), f32_dict(s), f32_dict(col)
    rd = f32 if storage else (lambda a: a)  # what a float32 field makes of an input
    env = Env(lib, device, m, n, nz)
    g = Grid(n, nz, m)
    for k in ("crx", "cry", "xfx", "yfx"):
        s[k] = np.zeros_like(s["pt"])
    dgrid_sw.fxadv(g, s["uc"], s["vc"], s["crx"], s["cry"], s["xfx"], s["yfx"], np.zeros_like(s["pt"]), np.zeros_like(s["pt"]), s["dt"])
    for k in ("crx", "cry", "xfx", "yfx"):
        s[k] = rd(s[k])
    errs = {}
    q, crx, cry = env.q3(s["pt"]), env.q3(s["crx"]), env.q3(s["cry"])
    for iord in (5, 6, 8):
        # inner x sweep of fvtp2d: origin (is, jsd), domain (n + 1, n + 6); inner y: origin (isd, js), domain (n + 6, n + 1)
        for cls, axis, c_q, c_np, metric, name in ((XPiecewiseParabolic, 0, crx, s["crx"], env.grid_data.dxa, "dxa"),
                                                   (YPiecewiseParabolic, 1, cry, s["cry"], env.grid_data.dya, "dya")):
            origin = (3, 0, 0) if axis == 0 else (0, 3, 0)
            domain = (n + 1, n + 6, nz) if axis == 0 else (n + 6, n + 1, nz)
            out = env.q3()
            cls(env.stencil_factory, metric, 0, iord, origin, domain)(q, c_q, out)
            if device != "cpu":
                torch.cuda.synchronize()
            ref = np.zeros_like(s["pt"])
            tr.ppm_flux(s["pt"], c_np, m[name], g, axis, iord, ref, origin, domain)
            W = tuple(slice(o, o + d) for o, d in zip(origin, domain))
            e = compare(rd(ref[W]), out.numpy()[W])
            errs[f"{'xy'[axis]}ppm{iord}"] = e
            if storage:
                assert out.numpy().dtype == np.float32 and np.array_equal(out.numpy()[W], ref[W].astype(np.float32)), (axis, iord, e)
            else:
                assert e == 0.0 if exact else e < 1e-14, (axis, iord, e)
            untouched = out.numpy().copy()
            untouched[W] = 0.0
            assert not untouched.any(), "written outside origin .. origin + domain"
    # DivergenceDamping on the synthetic winds (vorticity = a smooth field; ke = another)
    f = {k: s[k].copy() for k in ("u", "v", "va", "ua", "divgd", "vc", "uc")}
    f["vort_b"], f["delpc"] = np.zeros_like(s["pt"]), np.zeros_like(s["pt"])
    f["ke"] = rd(0.5 * (s["u"] ** 2 + s["v"] ** 2))
    f["wk"] = rd(1.0e-5 * s["pt"] * np.cos(s["u"] * 0.1))
    qf = {k: env.q3(a) for k, a in f.items()}
    rng = [np.random.default_rng(20240905 + d) for d in range(2)]

    def divdamp(f):
        damping.divergence_damping(g, f["u"], f["v"], f["va"], f["vort_b"], f["ua"], f["divgd"], f["vc"], f["uc"], f["delpc"], f["ke"],
                                   f["wk"], s["dt"], nord_k=col["nord"], d2_bg_k=col["d2_divg"], dddmp=DSW_CFG["dddmp"],
                                   d4_bg=DSW_CFG["d4_bg"], nord=DSW_CFG["nord"])
        return f

    noisy = [divdamp({k: f32_neighbours(a, r) for k, a in f.items()}) for r in rng] if storage else []
    op = DivergenceDamping(env.stencil_factory, env.qf, env.grid_data, env.damping, False, False, DSW_CFG["dddmp"], DSW_CFG["d4_bg"],
                           DSW_CFG["nord"], 0, env.kq(col["nord"]), env.kq(col["d2_divg"]))
    op(qf["u"], qf["v"], qf["va"], qf["vort_b"], qf["ua"], qf["divgd"], qf["vc"], qf["uc"], qf["delpc"], qf["ke"], qf["wk"], s["dt"])
    if device != "cpu":
        torch.cuda.synchronize()
    divdamp(f)
    B = _win(n, 0, 0, 1, 1)
    for k, W in (("vort_b", B), ("ke", B), ("delpc", B), ("divgd", B), ("uc", _win(n, 0, 0, 1, 0)), ("vc", _win(n, 0, 0, 0, 1))):
        if storage:
            errs["divdamp_" + k] = _staged_f32("divdamp_" + k, qf[k].numpy()[W][:, :, :nz], f[k][W][:, :, :nz],
                                               [x[k][W][:, :, :nz] for x in noisy], report)
            # (the nord passes run in LDS in double: the last pass's divergence, uc and vc are stored once)
            assert k not in ("divgd", "uc", "vc") or np.array_equal(qf[k].numpy()[W][:, :, :nz], f[k][W][:, :, :nz].astype(np.float32)), k
            continue
        e = compare(f[k][W][:, :, :nz], qf[k].numpy()[W][:, :, :nz], near_zero=1e-14 * float(np.abs(f[k][W]).max()))
        errs["divdamp_" + k] = e
        assert e == 0.0 if exact else e < 1.4e-10, (k, e)  # translate_divergencedamping.py:37
    # Sim1Solver with the inputs riem_solver3 prepares for it (riem_solver3.py:26-91), n_halo = 0 and 1
    with np.errstate(all="ignore"):
        pem = np.concatenate([np.full(s["delp"].shape[:2] + (1,), float(m["ptop"])), float(m["ptop"]) + np.cumsum(s["delp"][:, :, :nz], axis=2)], axis=2)
        pm = np.zeros_like(s["pt"])
        pm[:, :, :nz] = (pem[:, :, 1:] - pem[:, :, :-1]) / (np.log(pem[:, :, 1:]) - np.log(pem[:, :, :-1]))
    pm[~np.isfinite(pm)] = 1.0e4
    pem[~np.isfinite(pem)] = 1.0e4
    pm, pem = rd(pm), rd(pem)
    gm = rd(1.0 / (1.0 - s["cappa"]))
    dmass = s["delp"] * oc.RGRAV
    dmass[dmass <= 0] = 1.0  # (the allocator's extra level and unused halo cells)
    dmass = rd(dmass)
    dz0 = np.where(s["delz"] < 0, s["delz"], -100.0)
    for n_halo in (0, 1):
        f = dict(gamma=gm.copy(), cp3=s["cappa"].copy(), pe=np.zeros_like(s["pt"]), dm=dmass.copy(), pm=pm.copy(), pem=pem.copy(),
                 w=s["w"].copy(), dz=dz0.copy(), pt=np.where(s["pt"] > 0, s["pt"], 300.0), ws=rd(np.zeros(s["pt"].shape[:2]) + 0.01))
        q = {k: (env.q3(a) if a.ndim == 3 else env.q2(a)) for k, a in f.items()}
        from pace_amd.fv3core.stencils.sim1_solver import Sim1Solver

        op = Sim1Solver(env.stencil_factory, 0.05, n_halo)
        op(s["dt"], q["gamma"], q["cp3"], q["pe"], q["dm"], q["pm"], q["pem"], q["w"], q["dz"], q["pt"], q["ws"])
        if device != "cpu":
            torch.cuda.synchronize()

        def sim1(f):
            vertical.sim1_solve(f["w"], f["dm"], f["gamma"], f["dz"], f["pt"], f["pm"], f["pe"], f["pem"], f["ws"], f["cp3"], s["dt"],
                                0.05, (3 - n_halo, 3 + n + n_halo, 3 - n_halo, 3 + n + n_halo), nz)
            return f

        noisy = [sim1({k: f32_neighbours(a, r) for k, a in f.items()}) for r in rng] if storage else []
        sim1(f)
        Wd = (slice(3 - n_halo, 3 + n + n_halo), slice(3 - n_halo, 3 + n + n_halo))
        for k, nlev in (("w", nz), ("dz", nz), ("pe", nz + 1)):
            ref, got = f[k][Wd][:, :, :nlev], q[k].numpy()[Wd][:, :, :nlev]
            if storage:
                name = f"sim1_h{n_halo}_{k}"
                errs[name] = _staged_f32(name, got, ref, [x[k][Wd][:, :, :nlev] for x in noisy], report)
            else:
                e = compare(ref, got, near_zero=1e-5 * float(np.abs(ref).max()))
                errs[f"sim1_h{n_halo}_{k}"] = e
                assert e < 5e-6, (n_halo, k, e)  # the reference's Riem_Solver3 bound (the solver's only Translate-level users)
            untouched = q[k].numpy().copy() - (np.zeros_like(f[k]) if k == "pe" else (s["w"] if k == "w" else dz0))
            untouched[Wd] = 0.0
            assert not untouched[:, :, :nlev].any(), ("written outside the compute domain + n_halo", n_halo, k)
    return errs
