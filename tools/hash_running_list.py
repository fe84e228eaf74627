#!/usr/bin/env python3
"""sha256 of the raw output bytes of every case of tests/running_list_cases.py, as JSON on stdout.  Run on the commit whose bits
are to be kept (or on its library: TSIM_LIB=<path>) and store the output as tests/golden/running_list_parent.json;
tests/test_running_list_gpu.py recomputes and compares.

    python tools/hash_running_list.py > tests/golden/running_list_parent.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import running_list_cases as rl  # noqa: E402

json.dump({name: rl.digest(*run()) for name, run in rl.all_runs()}, sys.stdout, indent=1, sort_keys=True)
print()
