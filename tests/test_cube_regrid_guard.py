"""pace_cube_regrid under guard pages: the emulated cases of tests/test_cube_regrid.py in a child process in which every storage,
the dense buffer (allocated at its exact size: its first and last elements belong to items), the point table and the item table
with the prefix table behind it end at (over) or start right after (under) an inaccessible page (tests/guard.py).  An element
read or written one place outside its array, or a table row past the last, ends the child.  The emulation only: nothing of this
kind runs on a GPU."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT  # noqa: E402


@pytest.mark.parametrize("mode", ["over", "under"])
@pytest.mark.parametrize("what", ["check_kernel('cpu', (0, np.float32))", "check_kernel('cpu', (1, np.float64))"],
                         ids=["f64lib-dense32", "f32lib-dense64"])
def test_kernel_with_guard_pages(mode, what):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            f"import numpy as np\nimport guard, test_cube_regrid\nwith guard.guarded({mode!r}):\n    test_cube_regrid.{what}\n")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PACE_EMU_GUARD="1"))
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
