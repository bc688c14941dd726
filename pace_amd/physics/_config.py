"""PhysicsConfig (reference: physics/pace/physics/_config.py; defaults: util/pace/util/namelist.py NamelistDefaults)."""
import dataclasses
from typing import Optional, Tuple


@dataclasses.dataclass
class PhysicsConfig:
    dt_atmos: int = 0
    hydrostatic: bool = False
    npx: int = 0
    npy: int = 0
    npz: int = 0
    nwat: int = 0
    do_qa: bool = False  # (the reference's dataclass default; NamelistDefaults.do_qa, which from_namelist takes, is True)
    c_cracw: float = 0.8  # rain accretion efficiency
    c_paut: float = 0.5  # autoconversion cloud water to rain
    c_pgacs: float = 0.01  # snow to graupel "accretion" efficiency
    c_psaci: float = 0.05  # accretion: cloud ice to snow
    ccn_l: float = 300.0  # CCN over land (cm^-3)
    ccn_o: float = 100.0  # CCN over ocean (cm^-3)
    const_vg: bool = False
    const_vi: bool = False
    const_vr: bool = False
    const_vs: bool = False
    vs_fac: float = 1.0
    vg_fac: float = 1.0
    vi_fac: float = 1.0
    vr_fac: float = 1.0
    de_ice: bool = False
    layout: Tuple[int, int] = (1, 1)
    tau_imlt: float = 600.0  # cloud ice melting
    tau_i2s: float = 1000.0  # cloud ice to snow autoconversion
    tau_g2v: float = 1200.0  # graupel sublimation
    tau_v2g: float = 21600.0  # graupel deposition
    ql_mlt: float = 2.0e-3  # max cloud water from melted cloud ice
    qs_mlt: float = 1.0e-6  # max cloud water due to snow melt
    t_sub: float = 184.0  # min temperature for sublimation of cloud ice
    qi_gen: float = 1.82e-6  # max cloud ice generation
    qi_lim: float = 1.0  # cloud ice limiter
    qi0_max: float = 1.0e-4  # max cloud ice value (by other sources)
    rad_snow: bool = True
    rad_rain: bool = True
    dw_ocean: float = 0.10  # subgrid deviation over ocean
    dw_land: float = 0.15  # subgrid deviation over land
    tau_l2v: float = 300.0  # cloud water to vapor (evaporation)
    c2l_ord: int = 4
    do_sedi_heat: bool = False
    do_sedi_w: bool = True
    fast_sat_adj: bool = True
    qc_crt: float = 5.0e-8
    fix_negative: bool = True
    irain_f: int = 0
    mp_time: float = 225.0  # maximum microphysics time step (s)
    prog_ccn: bool = False
    qi0_crt: float = 8e-05
    qs0_crt: float = 0.003
    rh_inc: float = 0.2
    rh_inr: float = 0.3
    rthresh: float = 1e-05
    sedi_transport: bool = True
    use_ppm: bool = False
    vg_max: float = 16.0
    vi_max: float = 1.0
    vr_max: float = 16.0
    vs_max: float = 2.0
    z_slope_ice: bool = True
    z_slope_liq: bool = True
    tice: float = 273.16
    alin: float = 842.0
    clin: float = 4.8
    namelist_override: Optional[str] = None

    def __post_init__(self):
        if self.namelist_override is not None:
            raise NotImplementedError("namelist_override reads a Fortran namelist file: build the configuration by keyword or "
                                      "with from_namelist")

    @classmethod
    def from_namelist(cls, namelist) -> "PhysicsConfig":
        """From a namelist object that carries these fields as attributes (pace.util.Namelist); a field the namelist lacks
        takes NamelistDefaults' value (do_qa: True)."""
        values = {}
        for f in dataclasses.fields(cls):
            if f.name == "namelist_override":
                continue
            default = True if f.name == "do_qa" else f.default
            values[f.name] = getattr(namelist, f.name, default)
        return cls(**values)
