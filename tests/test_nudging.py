"""pace_amd.util.apply_nudging / get_nudging_tendencies (pace_amd/util/nudging.py).

* the float64 library against tests/golden/nudging_reference.npz, which tools/make_golden_nudging.py wrote by running the
  REFERENCE's functions on the inputs of tests/nudging_cases.py: the state's whole storage bit for bit (outside the compute
  domain it is the input), the tendencies' .view[:], their dims and units; get_nudging_tendencies leaves the state alone;
* the float32 library against the numpy restatement (tests/nudge_reference.py), bit for bit;
* one pace_nudge launch for three names, two for 33; preallocated tendencies are the ones returned and written;
* interpolation between two references against the restatement; weight 0 passes no second reference;
* timescale == timestep lands on the reference, and repeated nudging toward a constant reference contracts the difference by
  (1 - dt / tau) per call, each to within the rounding of the expression (`rounding_bound`);
* the refusals.

Every check is a function of the device: the CPU tier calls it with the emulation libraries, the GPU tier with the product's."""
import os
import sys
from datetime import timedelta

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import GOLDEN, build_emu, build_emu_f32  # noqa: E402
import nudge_reference  # noqa: E402
import nudging_cases as cases  # noqa: E402


def _libs(device):
    from pace_amd import _lib

    if device == "cpu":
        return [_lib.Library(build_emu()), _lib.Library(build_emu_f32())]
    return [_lib.load(), _lib.load(32)]


class CountingLib:
    """A library whose entry-point calls are counted (tests/test_diagnostics.py)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        self.calls.append(name)
        return self._lib.call(name, *args)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


class Setup:
    def __init__(self, lib, device, n=cases.N, nz=cases.NZ):
        import torch

        from pace_amd.util import CubedSphereCommunicator, NullComm, QuantityFactory, SubtileGridSizer

        self.lib = CountingLib(lib)
        self.device = device
        self.dtype = np.float32 if lib.real_bytes == 4 else np.float64
        self.factory = QuantityFactory(SubtileGridSizer(n, n, nz), device, torch.float32 if lib.real_bytes == 4 else torch.float64)
        self.communicator = CubedSphereCommunicator(NullComm(rank=0, total_ranks=6, fill_value=0.0), device=device, lib=self.lib)

    def quantities(self, arrays):
        return {name: self.factory.from_array(a, cases.VARIABLES[name][0], cases.VARIABLES[name][1]) for name, a in arrays.items()}

    def sync(self):
        if self.device != "cpu":
            import torch

            torch.cuda.synchronize()


TIMESCALES = {name: timedelta(seconds=cases.VARIABLES[name][3]) for name in cases.NAMES}
TIMESTEP = timedelta(seconds=cases.TIMESTEP_SECONDS)


def window(name):
    return cases.ORIGIN + cases.VARIABLES[name][2]


def check_against_the_reference(device):
    """The float64 library: the reference's bits."""
    from pace_amd.util import apply_nudging, get_nudging_tendencies

    s = Setup(_libs(device)[0], device)
    golden = dict(np.load(os.path.join(GOLDEN, "nudging_reference.npz"), allow_pickle=False))
    state_in, reference_in = cases.inputs()
    state, reference = s.quantities(state_in), s.quantities(reference_in)
    only = get_nudging_tendencies(state, reference, TIMESCALES, communicator=s.communicator)
    s.sync()
    for name in cases.NAMES:
        assert np.array_equal(_bits(state[name].numpy()), _bits(state_in[name]))
    applied = apply_nudging(state, reference, TIMESCALES, TIMESTEP, communicator=s.communicator)
    s.sync()
    assert s.lib.calls == ["pace_nudge", "pace_nudge"]  # one launch for the three names, each time
    assert list(applied) == list(only) == list(cases.NAMES)
    for name in cases.NAMES:
        want = state_in[name].copy()
        cases.view(name, want)[...] = golden[f"state_{name}"]
        assert np.array_equal(_bits(state[name].numpy()), _bits(want)), name
        assert np.array_equal(_bits(reference[name].numpy()), _bits(reference_in[name]))
        for tendencies in (only, applied):
            t = tendencies[name]
            assert np.array_equal(_bits(t.view[:].cpu().numpy()), _bits(golden[f"tendency_{name}"])), name
            assert tuple(t.dims) == tuple(golden[f"dims_{name}"]) == tuple(state[name].dims)
            assert t.units == str(golden[f"units_{name}"]) == state[name].units + " s^-1"
            # a storage of the state's layout, zero outside the compute domain
            assert t.data.shape == state[name].data.shape and t.data.stride() == state[name].data.stride()
            assert t.origin == state[name].origin and t.extent == state[name].extent
            outside = np.ones(t.data.shape, dtype=bool)
            cases.view(name, outside)[...] = False
            assert not t.numpy()[outside].any()


def check_against_the_restatement(device, which):
    """Either library, held and interpolated references, against tests/nudge_reference.py over the whole storage."""
    from pace_amd.util import apply_nudging

    s = Setup(_libs(device)[which], device)
    state_in, reference_in = cases.inputs(s.dtype)
    end_in = {name: (a + 0.5).astype(s.dtype).astype(np.float64) for name, a in reference_in.items()}
    for weight, with_end in ((0.0, False), (0.25, True), (1.0, True), (0.0, True)):
        state, reference, end = s.quantities(state_in), s.quantities(reference_in), s.quantities(end_in)
        passed = []
        real_call = s.lib._lib.call

        def spying_call(name, *args, passed=passed):
            passed.extend(bool(item.ref1) for item in args[1][:args[2]])
            return real_call(name, *args)

        s.lib._lib.call = spying_call
        try:
            tendencies = apply_nudging(state, reference, TIMESCALES, TIMESTEP, communicator=s.communicator,
                                       end_reference_state=end if with_end else None, weight=weight)
        finally:
            del s.lib._lib.call
        s.sync()
        assert passed == [with_end and weight != 0.0] * 3  # ref1 only with an end reference AND a weight that is not 0
        for name in cases.NAMES:
            f, r0, r1 = (a[name].astype(s.dtype) for a in (state_in, reference_in, end_in))
            want_f, want_t = nudge_reference.nudge(f, r0, r1 if passed[0] else None, window(name), cases.VARIABLES[name][3], weight,
                                                   cases.TIMESTEP_SECONDS, 1, np.zeros_like(f))
            assert np.array_equal(_bits(state[name].numpy()), _bits(want_f)), (name, weight)
            assert np.array_equal(_bits(tendencies[name].numpy()), _bits(want_t)), (name, weight)


def check_launches_and_preallocation(device):
    from pace_amd.util import apply_nudging, get_nudging_tendencies

    s = Setup(_libs(device)[0], device)
    state_in, reference_in = cases.inputs()
    state, reference = s.quantities(state_in), s.quantities(reference_in)
    mine = {name: s.factory.zeros(cases.VARIABLES[name][0], "anything") for name in cases.NAMES}
    pointers = {name: q.ptr for name, q in mine.items()}
    first = get_nudging_tendencies(state, reference, TIMESCALES, communicator=s.communicator, tendencies=mine)
    fresh = get_nudging_tendencies(state, reference, TIMESCALES, communicator=s.communicator)
    again = apply_nudging(state, reference, TIMESCALES, TIMESTEP, communicator=s.communicator, tendencies=mine)
    s.sync()
    assert s.lib.calls == ["pace_nudge"] * 3
    for name in cases.NAMES:
        assert first[name] is mine[name] and again[name] is mine[name] and mine[name].ptr == pointers[name]
        assert fresh[name] is not mine[name]
        assert np.array_equal(_bits(mine[name].numpy()), _bits(fresh[name].numpy())) and mine[name].numpy().any()
    # 33 names: two launches
    name = cases.NAMES[0]
    many_state = {f"v{m}": state[name] for m in range(33)}
    many_reference = {f"v{m}": reference[name] for m in range(33)}
    del s.lib.calls[:]
    many = get_nudging_tendencies(many_state, many_reference, {f"v{m}": timedelta(seconds=600.0 * (m + 1)) for m in range(33)},
                                  communicator=s.communicator)
    s.sync()
    assert s.lib.calls == ["pace_nudge"] * 2
    q, r = state[name].view[:].cpu().numpy(), reference[name].view[:].cpu().numpy()
    for m in (0, 31, 32):
        assert np.array_equal(_bits(many[f"v{m}"].view[:].cpu().numpy()), _bits((r - q) / (600.0 * (m + 1))))


U = 2.0 ** -53


def rounding_bound(q, r, ratio, new):
    """|computed - (q + (r - q) * ratio)| for new = fl(q + fl(fl(fl(r - q) / tau) * dt)), ratio = dt / tau, in double: the
    subtraction, the division and the multiplication each add at most u of |r - q| * ratio to the increment (3 u, and second
    order), the final addition at most u of the result."""
    return 1.001 * U * (3.0 * np.abs(r - q) * ratio + np.abs(new))


def check_properties(device):
    from pace_amd.util import apply_nudging

    s = Setup(_libs(device)[0], device)
    state_in, reference_in = cases.inputs()
    # timescale == timestep: the state lands on the reference
    state, reference = s.quantities(state_in), s.quantities(reference_in)
    apply_nudging(state, reference, {name: TIMESTEP for name in cases.NAMES}, TIMESTEP, communicator=s.communicator)
    s.sync()
    for name in cases.NAMES:
        q, r = cases.view(name, state_in[name]), cases.view(name, reference_in[name])
        new = cases.view(name, state[name].numpy())
        assert (np.abs(new - r) <= rounding_bound(q, r, 1.0, new)).all(), name
        assert not np.array_equal(new, q)
    # a constant reference: every call contracts the difference by (1 - dt / tau)
    name = cases.NAMES[0]
    tau, dt = 1800.0, 450.0
    state, reference = s.quantities(state_in), s.quantities(reference_in)
    r = cases.view(name, reference_in[name]).astype(np.longdouble)
    q = cases.view(name, state_in[name])
    for _ in range(4):
        apply_nudging(state, reference, {name: timedelta(seconds=tau)}, timedelta(seconds=dt), communicator=s.communicator)
        s.sync()
        new = cases.view(name, state[name].numpy()).copy()  # (on the CPU numpy() is the live storage)
        contracted = (q.astype(np.longdouble) - r) * (np.longdouble(1) - np.longdouble(dt) / np.longdouble(tau))
        error = np.abs((new.astype(np.longdouble) - r) - contracted).astype(np.float64)
        assert (error <= rounding_bound(q, r.astype(np.float64), dt / tau, new)).all()
        q = new
    assert np.abs(q - r.astype(np.float64)).max() < 0.32 * np.abs(cases.view(name, state_in[name]) - r.astype(np.float64)).max()


def check_refusals(device):
    import torch

    from pace_amd.util import QuantityFactory, SubtileGridSizer, apply_nudging, get_nudging_tendencies

    s = Setup(_libs(device)[0], device)
    state_in, reference_in = cases.inputs()
    state, reference = s.quantities(state_in), s.quantities(reference_in)
    comm = s.communicator

    def without(d, name):
        return {k: v for k, v in d.items() if k != name}

    name = cases.NAMES[1]
    for function, extra in ((apply_nudging, (TIMESTEP,)), (get_nudging_tendencies, ())):
        with pytest.raises(KeyError):  # the reference's: state[name]
            function(without(state, name), reference, TIMESCALES, *extra, communicator=comm)
        with pytest.raises(KeyError):
            function(state, without(reference, name), TIMESCALES, *extra, communicator=comm)
        with pytest.raises(KeyError):
            function(state, reference, TIMESCALES, *extra, communicator=comm, tendencies={})
        with pytest.raises(KeyError):
            function(state, reference, TIMESCALES, *extra, communicator=comm, end_reference_state=without(reference, name), weight=0.5)
        for weight in (-0.1, 1.1, float("nan")):
            with pytest.raises(ValueError, match="weight"):
                function(state, reference, TIMESCALES, *extra, communicator=comm, end_reference_state=reference, weight=weight)
        for seconds in (0.0, -5.0):
            with pytest.raises(ValueError, match="timescale"):
                function(state, reference, dict(TIMESCALES, **{name: timedelta(seconds=seconds)}), *extra, communicator=comm)
        # mixed layouts: a reference of another grid, of another level count, of other dims
        for n, nz in ((13, cases.NZ), (cases.N, cases.NZ + 1)):
            other = QuantityFactory(SubtileGridSizer(n, n, nz), device, torch.float64)
            odd = dict(reference, **{name: other.zeros(cases.VARIABLES[name][0], "m/s")})
            with pytest.raises(ValueError, match="layout"):
                function(state, odd, TIMESCALES, *extra, communicator=comm)
        plane = dict(reference, **{name: s.factory.zeros(["x", "y"], "m/s")})
        with pytest.raises(ValueError):
            function(state, plane, TIMESCALES, *extra, communicator=comm)
    # the other library's storage type
    single = QuantityFactory(SubtileGridSizer(cases.N, cases.N, cases.NZ), device, torch.float32)
    state32 = {k: single.zeros(cases.VARIABLES[k][0], "") for k in cases.NAMES}
    with pytest.raises(ValueError, match="storage type"):
        apply_nudging(state32, state32, TIMESCALES, TIMESTEP, communicator=comm, tendencies=state32)
    s.sync()
    assert s.lib.calls == []  # nothing was launched
    for k in cases.NAMES:
        assert np.array_equal(_bits(state[k].numpy()), _bits(state_in[k]))
    assert get_nudging_tendencies(state, reference, {}, communicator=comm) == {}


def test_exported_from_the_package():
    import pace_amd.util

    assert callable(pace_amd.util.apply_nudging) and callable(pace_amd.util.get_nudging_tendencies)


def test_golden_emulated():
    check_against_the_reference("cpu")


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_restatement_emulated(library):
    check_against_the_restatement("cpu", library)


def test_launches_and_preallocation_emulated():
    check_launches_and_preallocation("cpu")


def test_properties_emulated():
    check_properties("cpu")


def test_refusals_emulated():
    check_refusals("cpu")


@pytest.mark.gpu
def test_golden_on_the_gpu():
    check_against_the_reference("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_restatement_on_the_gpu(library):
    check_against_the_restatement("cuda", library)


@pytest.mark.gpu
def test_launches_properties_and_refusals_on_the_gpu():
    check_launches_and_preallocation("cuda")
    check_properties("cuda")
    check_refusals("cuda")
