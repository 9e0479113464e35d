"""bench.py's command line: `--full` exists and is off by default, and the options that select among the legs of a full run (`--legs`, `--extra`) are refused without
it instead of being ignored -- decided while the arguments are parsed, before anything touches a GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run(*args):
    return subprocess.run([sys.executable, BENCH] + list(args), capture_output=True, text=True, timeout=120)


def test_help_names_full():
    r = run("--help")
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_leg_selection_needs_full():
    for extra in (("--legs", "me"), ("--extra",)):
        r = run("--gpus", "1", "--steps", "2", "--warmup", "1", *extra)
        assert r.returncode == 2 and "--full" in r.stderr, (extra, r.returncode, r.stderr[-300:])
