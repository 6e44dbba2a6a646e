#!/usr/bin/env python3
"""bench.py's run with SHS_OPT_LEGACY_GROUP_SPANS forced to 0 on every context (a tile group's pair pass
walks whole clipped boxes, as before the option existed): the fallback's timing against the default.
Takes bench.py's arguments, prints its line.  Run from the repository root:
    python tools/bench_spans_off.py --gpus 1 [--config c1]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "leisure-software-renderer_amd"))

import bench  # noqa: E402
import shs_gpu  # noqa: E402

_init = shs_gpu.Context.__init__


def _init_off(self, *a, **kw):
    _init(self, *a, **kw)
    self.set_group_spans(False)


shs_gpu.Context.__init__ = _init_off

if __name__ == "__main__":
    bench.main()
