"""The host tree stage of HDBSCAN (csrc/hdbscan_tree.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
program.

hdbscan_tree.cpp indexes a dozen arrays with row numbers that come from the caller's edges.  tests/hdbscan_tree_driver.cpp (its
own ``main``) is compiled together with it by the host ``g++`` with the sanitizers on, fed case files — the small cases, a
golden case, and the malformed edges —, and must exit 0 without a sanitizer report and print exactly what the restatement
(tests/hdbscan_cases.tree_labels_ref) gives for the same case.  Host code only: nothing is loaded into the Python process, no GPU
is involved, and the test is not marked ``gpu``."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hdbscan_cases as hc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# a report of either sanitizer (a leak included) ends the run with a non-zero status
SAN_ENV = {"ASAN_OPTIONS": "abort_on_error=0:detect_leaks=1:exitcode=23", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no host g++")
    out = tmp_path_factory.mktemp("ht_driver")
    probe = out / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([gxx, *FLAGS, str(probe), "-o", str(out / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(out / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build or run a program with -fsanitize=address,undefined (sanitizer runtime missing): "
                    + (r.stderr.strip().splitlines() or ["?"])[-1])
    exe = out / "hdbscan_tree_driver"
    r = subprocess.run([gxx, *FLAGS, "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "hdbscan_tree_driver.cpp"),
                        os.path.join(REPO, "text_similarity_amd", "csrc", "hdbscan_tree.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def _run(driver, tmp_path, name, frm, to, w2, n, mcs):
    frm, to = np.asarray(frm, dtype="<i4"), np.asarray(to, dtype="<i4")
    w2 = np.asarray(w2, dtype="<f4")
    assert frm.shape == to.shape == w2.shape == (max(n - 1, 0),)
    case = tmp_path / f"{name}.case"
    case.write_bytes(b"HTC1" + struct.pack("<qiq", n, mcs, frm.size) + frm.tobytes() + to.tobytes() + w2.tobytes())
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    env.update(SAN_ENV)
    r = subprocess.run([driver, str(case)], capture_output=True, text=True, env=env, timeout=300)
    report = [ln for ln in r.stderr.splitlines() if "Sanitizer" in ln or "runtime error" in ln]
    assert r.returncode == 0 and not report and not r.stderr.strip(), (name, r.returncode, r.stderr[-3000:])
    want = hc.tree_labels_ref(frm, to, w2, n, mcs) if mcs >= 2 and n >= 1 else None
    if want is None:
        assert r.stdout == "rc 1\n", (name, r.stdout[:200])
    else:
        labels, k = want
        assert r.stdout == f"rc 0\nclusters {k}\nlabels" + "".join(f" {int(v)}" for v in labels) + "\n", (name, r.stdout[:200])


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (rows, mcs, ms) in hc.small_cases().items():
        out[name] = (rows.shape[0], mcs, hc.mst_ref(rows, hc.core2_ref(rows, ms)))
    rows, mcs, ms = hc.golden_case(2)
    out["golden2"] = (rows.shape[0], mcs, hc.mst_ref(rows, hc.core2_ref(rows, ms)))
    return out


def test_small_and_golden_cases(driver, tmp_path, cases):
    for name, (n, mcs, edges) in cases.items():
        for m in sorted({mcs, 2, 3, n, n + 1}):
            _run(driver, tmp_path, f"{name}_{m}", *edges, n, m)
    e = np.zeros((0,), dtype=np.int32)
    _run(driver, tmp_path, "one_row", e, e, e.astype(np.float32), 1, 2)


def test_malformed_cases(driver, tmp_path, cases):
    n, mcs, (frm, to, w2) = cases["mcs2"]
    k = 0
    for at in (0, 5, n - 2):
        for val in (-1, n, n + 1, (1 << 31) - 1, -(1 << 31), 1 << 30):
            for which in (0, 1):
                f, t = frm.copy(), to.copy()
                (f, t)[which][at] = val
                _run(driver, tmp_path, f"bad{k}", f, t, w2, n, mcs)
                k += 1
    t = to.copy()
    t[7] = t[6]
    _run(driver, tmp_path, "cycle", frm, t, w2, n, mcs)
    _run(driver, tmp_path, "loops", to, to, w2, n, mcs)
    _run(driver, tmp_path, "all_zero", np.zeros_like(frm), np.zeros_like(to), w2, n, mcs)
    for bad_w in (np.nan, -1.0, np.inf, -np.inf):          # the weights only order the merges: any float is a legal weight
        w = w2.copy()
        w[::3] = bad_w
        _run(driver, tmp_path, f"w_{bad_w}", frm, to, w, n, mcs)
    _run(driver, tmp_path, "mcs1", frm, to, w2, n, 1)
    _run(driver, tmp_path, "mcs_neg", frm, to, w2, n, -5)
    e = np.zeros((0,), dtype=np.int32)
    _run(driver, tmp_path, "n0", e, e, e.astype(np.float32), 0, 2)
    _run(driver, tmp_path, "n_neg", e, e, e.astype(np.float32), -1, 2)
