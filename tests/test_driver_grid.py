"""DriverGridData and the grid terms it is made of (MetricTerms.vlon, .vlat, .edge_vect_*) against what the reference's own
MetricTerms produced at C12 on six tiles (tests/golden/drivergrid_c12.npz, tools/make_golden_fvupdatephys.py).  CPU only.

Bounds as tests/test_gridgen.py applies them to every metric term: 2e-11 of the term's largest magnitude over the whole storage,
the reference's 1e8 "no value here" markers at exactly the same places."""
import numpy as np
import pytest

from helpers import golden
from test_gridgen import TOL

N, NZ = 12, 79


@pytest.fixture(scope="module")
def ref():
    return golden("drivergrid_c12.npz")


def close(r, g, what):
    assert r.shape == g.shape, (what, r.shape, g.shape)
    marker = np.abs(r) >= 1.0e7
    assert np.array_equal(marker, np.abs(g) >= 1.0e7), (what, "the 1e8 markers sit elsewhere")
    assert np.array_equal(r[marker], g[marker]), (what, "markers differ")
    both_nan = np.isnan(r) & np.isnan(g)
    keep = ~marker & ~both_nan
    scale = float(np.abs(r[keep]).max())
    err = float(np.abs(g[keep] - r[keep]).max())
    assert err <= TOL * scale, (what, err / scale)


def test_metric_terms_gain_the_driver_terms(ref):
    from pace_amd.util import gridgen

    tiles = gridgen.tiles(N, NZ)
    for t in range(6):
        for k in ("vlon", "vlat", "edge_vect_w", "edge_vect_e", "edge_vect_s", "edge_vect_n"):
            close(ref[f"{k}_tile{t}"], np.asarray(tiles[t][k]), (t, k))
        for k in ("edge_vect_w", "edge_vect_e", "edge_vect_s", "edge_vect_n"):
            g = np.asarray(tiles[t][k])
            assert (g[:2] == 1.0e8).all() and (g[-3:-1] == 1.0e8).all() and g[-1] == 0.0, (t, k)
            assert g[2] == g[3] and g[-4] == g[-5], (t, k, "the entries next to the corners copy their neighbours")
        # es1, ew2 where the operators read them: the south faces of (nx, ny + 1), the west faces of (nx + 1, ny)
        close(ref[f"es1_tile{t}"][3:15, 3:16], np.asarray(tiles[t]["es1"])[3:15, 3:16], (t, "es1"))
        close(ref[f"ew2_tile{t}"][3:16, 3:15], np.asarray(tiles[t]["ew2"])[3:16, 3:15], (t, "ew2"))


def test_driver_grid_data_from_metric_terms(ref):
    """new_from_metric_terms on all six tiles: 16 fields, 2-D device Quantities and 1-D tensors, with the TRUE vlat (the
    reference's constructor passes vlon twice, helper.py:683)."""
    import types

    import torch

    from pace_amd.util import QuantityFactory, SubtileGridSizer
    from pace_amd.util.grid import DriverGridData, MetricTerms

    sizer = SubtileGridSizer.from_tile_params(nx_tile=N, ny_tile=N, nz=NZ, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
    qf = QuantityFactory(sizer, device="cpu")
    assert len(DriverGridData.FIELDS) == 16
    for t in range(6):
        mt = MetricTerms(qf, types.SimpleNamespace(rank=t))
        info = DriverGridData.new_from_metric_terms(mt)
        for m in range(3):
            close(ref[f"vlon_tile{t}"][:, :, m], getattr(info, f"vlon{m + 1}").numpy(), (t, "vlon", m))
            close(ref[f"vlat_tile{t}"][:, :, m], getattr(info, f"vlat{m + 1}").numpy(), (t, "vlat", m))
            close(ref[f"es1_tile{t}"][3:15, 3:16, m], getattr(info, f"es1_{m + 1}").numpy()[3:15, 3:16], (t, "es1", m))
            close(ref[f"ew2_tile{t}"][3:16, 3:15, m], getattr(info, f"ew2_{m + 1}").numpy()[3:16, 3:15], (t, "ew2", m))
            assert getattr(info, f"vlon{m + 1}").dims == ("x", "y")
        assert not np.array_equal(info.vlat1.numpy(), info.vlon1.numpy())
        for k in ("edge_vect_w", "edge_vect_e", "edge_vect_s", "edge_vect_n"):
            e = getattr(info, k)
            assert torch.is_tensor(e) and e.dim() == 1 and e.shape[0] == N + 7
            close(ref[f"{k}_tile{t}"], e.numpy(), (t, k))


def test_new_from_grid_variables_checks_its_arguments(ref):
    from pace_amd.util import QuantityFactory, SubtileGridSizer
    from pace_amd.util.grid import DriverGridData

    sizer = SubtileGridSizer.from_tile_params(nx_tile=N, ny_tile=N, nz=NZ, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
    qf = QuantityFactory(sizer, device="cpu")
    kw = {k: ref[f"{k}_tile0"] for k in ("vlon", "vlat", "es1", "ew2", "edge_vect_w", "edge_vect_e", "edge_vect_s", "edge_vect_n")}
    with pytest.raises(ValueError):
        DriverGridData.new_from_grid_variables(**kw)
    with pytest.raises(ValueError):
        DriverGridData.new_from_grid_variables(**dict(kw, vlon=kw["vlon"][:, :, :2]), quantity_factory=qf)
    # the reference's 2-D edge_vect_w / _e (constant along i) are taken too
    two_d = np.repeat(kw["edge_vect_w"][None, :], N + 7, axis=0)
    info = DriverGridData.new_from_grid_variables(**dict(kw, edge_vect_w=two_d), quantity_factory=qf)
    assert np.array_equal(info.edge_vect_w.numpy(), kw["edge_vect_w"])
