"""bench.py's command line (no GPU: argument parsing only).  A plain run measures its headline and nothing else; `--full` adds the
side measurements, each of which its `--no-*` switch still drops."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = ("no_gemm_timing", "no_ref_numerics", "no_h2d", "no_configs4", "no_cpu_baseline")


def _parse(*argv):
    """bench.parse() on `argv` in a fresh interpreter (importing bench.py sets process environment)."""
    code = ("import json, sys; sys.argv = ['bench.py'] + json.loads(sys.argv[1]); import bench; a = bench.parse(); "
            "print(json.dumps({k: getattr(a, k) for k in ('full',) + %r}))" % (SIDE,))
    r = subprocess.run([sys.executable, "-c", code, json.dumps(list(argv))], capture_output=True, text=True, timeout=300, cwd=ROOT)
    return r.returncode, (json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else r.stderr)


def test_plain_run_switches_every_side_measurement_off():
    rc, a = _parse("--gpus", "1", "--steps", "3", "--warmup", "1")
    assert rc == 0, a
    assert a["full"] is False and all(a[k] is True for k in SIDE), a


def test_full_run_keeps_the_side_measurements_and_their_switches():
    rc, a = _parse("--full")
    assert rc == 0, a
    assert a["full"] is True and all(a[k] is False for k in SIDE), a
    rc, a = _parse("--full", "--no-h2d", "--no-cpu-baseline")
    assert rc == 0, a
    assert a["no_h2d"] is True and a["no_cpu_baseline"] is True and a["no_gemm_timing"] is False and a["no_configs4"] is False, a


def test_gemm_breakdown_needs_full():
    rc, err = _parse("--gemm-breakdown")
    assert rc == 2 and "--gemm-breakdown" in err and "--full" in err, err
    rc, a = _parse("--gemm-breakdown", "--full")
    assert rc == 0, a
