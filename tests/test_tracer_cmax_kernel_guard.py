"""The launches of the tracer advection's Courant-number sub-cycling under guard pages: the emulated cases of
tests/test_tracer_cmax_kernel.py in a child process in which every storage -- the Courant numbers, the sine plane, the fields of
the `_levels` stencils, the metric terms, cmax, the tables, the counts and ksplt -- ends at (over) or starts right after (under)
an inaccessible page (tests/guard.py).  An element read or written one place outside its array ends the child.  The emulation
only: nothing of this kind runs on a GPU."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT  # noqa: E402


@pytest.mark.parametrize("mode", ["over", "under"])
@pytest.mark.parametrize("what", ["check_cmax('cpu', 0)", "check_cmax('cpu', 1)", "check_order('cpu')", "check_subcycles('cpu', 0)",
                                  "check_subcycles('cpu', 1)", "check_levels('cpu', 0)", "check_levels('cpu', 1)", "check_refusals('cpu')"],
                         ids=["cmax-f64lib", "cmax-f32lib", "order", "subcycles-f64lib", "subcycles-f32lib", "levels-f64lib", "levels-f32lib",
                              "refusals"])
def test_kernel_with_guard_pages(mode, what):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            f"import guard, test_tracer_cmax_kernel\nwith guard.guarded({mode!r}):\n    test_tracer_cmax_kernel.{what}\n")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PACE_EMU_GUARD="1"))
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
