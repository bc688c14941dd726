"""Namelist-style configuration dataclasses: the subset of fv3core/pace/fv3core/_config.py:59-476 the
acoustic step reads, with the reference's field names and defaults for the baroclinic test case."""
import dataclasses
from collections.abc import Mapping
from typing import Any, Dict, Optional, Tuple


@dataclasses.dataclass
class RiemannConfig:
    p_fac: float = 0.05
    a_imp: float = 1.0
    use_logp: bool = False
    beta: float = 0.0


@dataclasses.dataclass
class DGridShallowWaterLagrangianDynamicsConfig:
    dddmp: float = 0.5
    d2_bg: float = 0.0
    d2_bg_k1: float = 0.2
    d2_bg_k2: float = 0.1
    d4_bg: float = 0.15
    ke_bg: float = 0.0
    nord: int = 3
    n_sponge: int = 48
    grid_type: int = 0
    d_ext: float = 0.0
    inline_q: bool = False
    hord_dp: int = 6
    hord_tm: int = 6
    hord_mt: int = 6
    hord_vt: int = 6
    do_f3d: bool = False
    do_skeb: bool = False
    d_con: float = 1.0
    vtdm4: float = 0.06
    do_vort_damp: bool = True
    hydrostatic: bool = False
    convert_ke: bool = False


@dataclasses.dataclass
class AcousticDynamicsConfig:
    n_split: int = 1
    k_split: int = 1
    nord: int = 3
    d_con: float = 1.0
    d_ext: float = 0.0
    beta: float = 0.0
    use_logp: bool = False
    hydrostatic: bool = False
    rf_fast: bool = True
    rf_cutoff: float = 3000.0
    tau: float = 10.0
    p_fac: float = 0.05
    hord_tm: int = 6
    grid_type: int = 0
    delt_max: float = 0.002
    breed_vortex_inline: bool = False
    use_old_omega: bool = True
    d_grid_shallow_water: DGridShallowWaterLagrangianDynamicsConfig = dataclasses.field(
        default_factory=DGridShallowWaterLagrangianDynamicsConfig
    )
    riemann: RiemannConfig = dataclasses.field(default_factory=RiemannConfig)


@dataclasses.dataclass(frozen=True)
class SatAdjustConfig:
    """fv3core/pace/fv3core/_config.py:16-40, with the defaults of util/pace/util/namelist.py:22-51."""

    hydrostatic: bool = False
    rad_snow: bool = True
    rad_rain: bool = True
    rad_graupel: bool = True
    tintqs: bool = False
    sat_adj0: float = 0.90
    ql_gen: float = 1.0e-3
    qs_mlt: float = 1.0e-6
    ql0_max: float = 2.0e-3
    t_sub: float = 184.0
    qi_gen: float = 1.82e-6
    qi_lim: float = 1.0
    qi0_max: float = 1.0e-4
    dw_ocean: float = 0.10
    dw_land: float = 0.15
    icloud_f: int = 0
    cld_min: float = 0.05
    tau_i2s: float = 1000.0
    tau_v2l: float = 90.0
    tau_r2g: float = 900.0
    tau_l2r: float = 900.0
    tau_l2v: float = 300.0
    tau_imlt: float = 600.0
    tau_smlt: float = 900.0


_SAT_ADJUST_FIELDS = tuple(f.name for f in dataclasses.fields(SatAdjustConfig) if f.name != "hydrostatic")


@dataclasses.dataclass
class DynamicalCoreConfig:
    layout: Tuple[int, int] = (1, 1)
    npx: int = 13
    npy: int = 13
    npz: int = 79
    dt_atmos: float = 225.0
    k_split: int = 1
    n_split: int = 1
    acoustic_dynamics: AcousticDynamicsConfig = dataclasses.field(default_factory=AcousticDynamicsConfig)
    # what DynamicalCore itself reads (fv3core/pace/fv3core/_config.py:150-420; defaults = util/pace/util/namelist.py:10-70
    # with the baseline case's values for the ones it sets)
    nwat: int = 6
    moist_phys: bool = True
    hydrostatic: bool = False
    z_tracer: bool = True
    inline_q: bool = False
    adiabatic: bool = False
    check_negative: bool = False
    consv_te: float = 0.0
    rf_fast: bool = True
    tau: float = 10.0
    grid_type: int = 0
    hord_tr: int = 8
    c2l_ord: int = 4
    nf_omega: int = 1
    fill: bool = True
    kord_tm: int = -9
    kord_tr: int = 9
    kord_wz: int = 9
    kord_mt: int = 9
    do_sat_adj: bool = False
    # the saturation adjustment's namelist (util/pace/util/namelist.py:22-51)
    tau_r2g: float = 900.0
    tau_smlt: float = 900.0
    tau_imlt: float = 600.0
    tau_i2s: float = 1000.0
    tau_l2r: float = 900.0
    sat_adj0: float = 0.90
    ql_gen: float = 1.0e-3
    qs_mlt: float = 1.0e-6
    ql0_max: float = 2.0e-3
    t_sub: float = 184.0
    qi_gen: float = 1.82e-6
    qi_lim: float = 1.0
    qi0_max: float = 1.0e-4
    rad_snow: bool = True
    rad_rain: bool = True
    rad_graupel: bool = True
    tintqs: bool = False
    dw_ocean: float = 0.10
    dw_land: float = 0.15
    icloud_f: int = 0
    cld_min: float = 0.05
    tau_l2v: float = 300.0
    tau_v2l: float = 90.0
    # the dry convective adjustment's time scale in seconds (util/pace/util/namelist.py: fv_sg_adj = -1, off)
    fv_sg_adj: int = -1
    # an extension: the tracer advection sub-cycles level k int(1 + cmax(k)) times, cmax(k) the level's largest Courant number
    # over the globe, as the Fortran tracer_2d_1L does; false: the reference's fixed three sub-cycles on every level
    tracer_courant_subcycling: bool = False
    # fields of the reference's flat configuration that nothing here reads: carried so that its files load and round-trip
    # (defaults: util/pace/util/namelist.py NamelistDefaults)
    ntiles: int = 6
    do_qa: bool = True
    tau_g2r: float = 600.0
    tau_g2v: float = 1200.0
    tau_v2g: float = 21600.0
    ql_mlt: float = 2.0e-3
    regional: bool = False
    m_split: int = 0
    namelist_override: Optional[str] = None

    def __post_init__(self):
        if self.namelist_override is not None:
            raise NotImplementedError("namelist_override reads a Fortran namelist file: build the configuration by keyword or "
                                      "with from_namelist_dict")

    @classmethod
    def from_namelist_dict(cls, values: Dict[str, Any]) -> "DynamicalCoreConfig":
        """From the reference's FLAT dycore configuration (the `dycore_config` section of a driver yaml file, the fields of
        fv3core/pace/fv3core/_config.py:150-420): every key is set in every place that keeps a field of that name -- this class,
        AcousticDynamicsConfig, DGridShallowWaterLagrangianDynamicsConfig, RiemannConfig -- so that the copies of nord, d_con,
        hord_tm, p_fac, hydrostatic, grid_type, n_split, k_split, ... agree.  Strict: a key that none of them has raises
        ValueError and names itself, and so does a value of the wrong type (an int is taken for a float field)."""
        config = cls()
        places = (config, config.acoustic_dynamics, config.acoustic_dynamics.d_grid_shallow_water, config.acoustic_dynamics.riemann)
        for key, value in values.items():
            found = False
            for place in places:
                field = {f.name: f for f in dataclasses.fields(place)}.get(key)
                if field is None or key in _NESTED:
                    continue
                setattr(place, key, strict_value(f"dycore_config.{key}", field.type, value))
                found = True
            if not found:
                raise ValueError(f"dycore_config has no setting {key!r}")
        config.__post_init__()
        return config

    @classmethod
    def from_f90nml(cls, namelist) -> "DynamicalCoreConfig":
        """From a namelist as a host model holds it (fv3core/pace/fv3core/_config.py:288-290 with util/pace/util/namelist.py:452-479):
        any mapping, an f90nml.Namelist included, in one of the two forms SubtileGridSizer.from_namelist takes --

            top-level nx_tile, nz, layout, dt_atmos and a `dycore_config` group   (the reference's test_init_from_geos.py)
            Fortran groups, with npx, npy, npz, layout in `fv_core_nml`           (dt_atmos in whichever group holds it)

        The groups are flattened (a key in two groups: ValueError), keys that no configuration class knows are dropped as the
        reference's filter drops them, and the rest goes through from_namelist_dict: a known key of the wrong type still raises."""
        flat = namelist_to_flatish_dict(namelist)
        if "fv_core_nml" in namelist.keys():
            core = namelist["fv_core_nml"]
            npx, npy, npz, layout = core["npx"], core["npy"], core["npz"], core["layout"]
        elif "nx_tile" in namelist.keys():
            npx, npy, npz, layout = namelist["nx_tile"] + 1, namelist["nx_tile"] + 1, namelist["nz"], namelist["layout"]
        else:
            raise KeyError("Namelist format is unrecognized, expected to find nx_tile or fv_core_nml")
        places = (cls, AcousticDynamicsConfig, DGridShallowWaterLagrangianDynamicsConfig, RiemannConfig)
        known = {f.name for place in places for f in dataclasses.fields(place)} - set(_NESTED) - set(_DERIVED)
        config = cls.from_namelist_dict({key: value for key, value in flat.items() if key in known})
        config.npx, config.npy, config.npz = (strict_value(f"namelist.{k}", int, v) for k, v in (("npx", npx), ("npy", npy), ("npz", npz)))
        config.layout = strict_value("namelist.layout", Tuple[int, int], layout)
        config.dt_atmos = strict_value("namelist.dt_atmos", float, flat["dt_atmos"])
        return config

    @property
    def n_sponge(self) -> int:
        return self.acoustic_dynamics.d_grid_shallow_water.n_sponge

    @property
    def do_dry_convective_adjustment(self) -> bool:
        """fv3core/pace/fv3core/_config.py: fv_sg_adj > 0."""
        return self.fv_sg_adj > 0

    @property
    def sat_adjust(self) -> SatAdjustConfig:
        """fv3core/pace/fv3core/_config.py:437-464."""
        return SatAdjustConfig(hydrostatic=self.hydrostatic, **{n: getattr(self, n) for n in _SAT_ADJUST_FIELDS})

    @property
    def remapping(self):
        return RemappingConfig(fill=self.fill, kord_tm=self.kord_tm, kord_tr=self.kord_tr, kord_wz=self.kord_wz,
                               kord_mt=self.kord_mt, do_sat_adj=self.do_sat_adj, hydrostatic=self.hydrostatic,
                               sat_adjust=self.sat_adjust)

    @property
    def d_grid_shallow_water(self):
        return self.acoustic_dynamics.d_grid_shallow_water

    @property
    def riemann(self):
        return self.acoustic_dynamics.riemann


_NESTED = ("acoustic_dynamics", "d_grid_shallow_water", "riemann")
# what from_f90nml takes from the grid's keys and not from a dycore setting of that name
_DERIVED = ("layout", "npx", "npy", "npz", "dt_atmos", "ntiles")


def namelist_to_flatish_dict(namelist) -> Dict[str, Any]:
    """util/pace/util/namelist.py:463-479: the keys of every group of a namelist side by side with its top-level keys (one
    level: a group inside a group stays a value).  A key that two groups hold, or a group and the top level before it, raises."""
    flat = {}
    for key, value in dict(namelist).items():
        if isinstance(value, Mapping):
            for subkey, subvalue in value.items():
                if subkey in flat:
                    raise ValueError("Cannot flatten this namelist, duplicate keys: " + subkey)
                flat[subkey] = subvalue
        else:
            flat[key] = value
    return flat


@dataclasses.dataclass(frozen=True)
class RemappingConfig:
    """fv3core/pace/fv3core/_config.py:42-56."""

    fill: bool = True
    kord_tm: int = -9
    kord_tr: int = 9
    kord_wz: int = 9
    kord_mt: int = 9
    do_sat_adj: bool = False
    hydrostatic: bool = False
    sat_adjust: SatAdjustConfig = dataclasses.field(default_factory=SatAdjustConfig)


def strict_value(where: str, kind, value):
    """`value` as a field of type `kind` (bool, int, float, str, Tuple[int, int], Optional[str]) takes it, or a ValueError that
    names the setting: the strictness of the reference's dacite.Config(strict=True) for the types a configuration file holds."""
    if kind in (Optional[str], "Optional[str]"):
        if value is None or isinstance(value, str):
            return value
    elif kind in (Tuple[int, int], "Tuple[int, int]"):
        if isinstance(value, (list, tuple)) and len(value) == 2 and all(isinstance(x, int) and not isinstance(x, bool) for x in value):
            return tuple(value)
    elif kind in (bool, "bool"):
        if isinstance(value, bool):
            return value
    elif kind in (int, "int"):
        if isinstance(value, int) and not isinstance(value, bool):
            return value
    elif kind in (float, "float"):
        if isinstance(value, (int, float)) and not isinstance(value, bool):
            return float(value)
    elif kind in (str, "str"):
        if isinstance(value, str):
            return value
    else:
        return value
    raise ValueError(f"{where} = {value!r}: expected {getattr(kind, '__name__', kind)}")
