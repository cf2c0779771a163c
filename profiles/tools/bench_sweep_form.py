"""bench.py with kernel 5's sweep form forced (DDH.set_sweep_form) on every DDH it builds; bench.py itself has no such switch.
usage: bench_sweep_form.py FORM [bench.py arguments]      FORM: 0 auto, 1 matrix, 2 element-lane; ignored by plans that are not kernel 5"""
import runpy
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

import cuddhelmholtz_amd as cd  # noqa: E402

form = int(sys.argv[1])
_init = cd.DDH.__init__


def init(self, *a, **kw):
    _init(self, *a, **kw)
    if form and self.info()["kernel"] == 5:
        self.set_sweep_form(form)
    print(f"bench_sweep_form: kernel {self.info()['kernel']}, sweep form {self.sweep_form()}", file=sys.stderr)


cd.DDH.__init__ = init
sys.argv = [str(ROOT / "bench.py")] + sys.argv[2:]
runpy.run_path(sys.argv[0], run_name="__main__")
