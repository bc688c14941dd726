"""pace_rayleigh_super under guard pages: the emulated cases of tests/test_rayleigh_kernel.py in a child process in which every
storage -- u, v, w, pt and the six metric planes -- ends at (over) or starts right after (under) an inaccessible page
(tests/guard.py).  An element read or written one place outside its array ends the child.  The emulation only: nothing of this
kind runs on a GPU."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT  # noqa: E402


@pytest.mark.parametrize("mode", ["over", "under"])
@pytest.mark.parametrize("what", ["check_kernel('cpu', 0)", "check_kernel('cpu', 1)", "check_specials('cpu')", "check_invariant('cpu')",
                                  "check_refusals('cpu')"],
                         ids=["f64lib", "f32lib", "specials", "invariant", "refusals"])
def test_kernel_with_guard_pages(mode, what):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            f"import guard, test_rayleigh_kernel\nwith guard.guarded({mode!r}):\n    test_rayleigh_kernel.{what}\n")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PACE_EMU_GUARD="1"))
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
