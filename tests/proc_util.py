"""Running a multi-process job (torchrun + ranks) from a test with a hard time limit.

`torch.distributed.run` starts every rank in its OWN session (subprocess_handler: start_new_session=True), so killing the
launcher's process group does not reach the ranks - and orphaned ranks keep the launcher's stdout / stderr pipes open, so a
`communicate()` after the kill never returns (seen: a test whose job hung waited on the dead launcher's pipes until the
box's time limit).  `run_job` therefore collects the launcher's descendants BEFORE it kills anything, kills those exact
pids, and bounds the final read of the pipes as well.  The launch helpers of the GPU tests sit on top of it, once:
`free_port`, `launch_ranks` (a tests/mp_*.py script under torchrun), `bench_line` (`bench.py --full` and its contract line).
"""
import json
import os
import signal
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class JobTimeout(Exception):
    def __init__(self, timeout, stdout, stderr, killed):
        super().__init__(f"job did not finish in {timeout} s")
        self.timeout, self.stdout, self.stderr, self.killed = timeout, stdout, stderr, killed


def _descendants(pid):
    import psutil

    try:
        return psutil.Process(pid).children(recursive=True)
    except psutil.Error:
        return []


def run_job(cmd, env=None, timeout=300, cwd=None):
    """-> CompletedProcess, or raises JobTimeout (after the launcher AND every descendant have been killed)."""
    import psutil

    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd,
                         env={**os.environ, **(env or {})}, start_new_session=True)
    try:
        out, err = p.communicate(timeout=timeout)
        return subprocess.CompletedProcess(cmd, p.returncode, out, err)
    except subprocess.TimeoutExpired:
        pass
    procs = _descendants(p.pid)          # before the launcher dies: afterwards its children belong to init
    for q in procs + _descendants(p.pid):
        try:
            q.send_signal(signal.SIGKILL)
        except psutil.Error:
            pass
    try:
        os.killpg(p.pid, signal.SIGKILL)
    except ProcessLookupError:
        pass
    psutil.wait_procs(procs, timeout=20)
    try:
        out, err = p.communicate(timeout=20)
    except subprocess.TimeoutExpired:    # something still holds the pipes: give up on the output, not on the test run
        for f in (p.stdout, p.stderr):
            try:
                f.close()
            except OSError:
                pass
        out, err = "", "(output unavailable: the pipes were still held after the kill)"
    raise JobTimeout(timeout, out or "", err or "", [q.pid for q in procs])


def run_job_or_fail(cmd, env=None, timeout=300):
    """`run_job` from the repository's root for a test: on a hang EVERY process of the job is killed and the test FAILS with
    the output tails - it never waits on orphaned ranks' pipes, and a deadlock is red, not a skip."""
    import pytest

    try:
        return run_job(cmd, env, timeout, cwd=ROOT)
    except JobTimeout as e:
        pytest.fail(f"{' '.join(cmd[-3:])} did not finish in {timeout} s; killed pids {e.killed}.  stdout tail: "
                    f"{e.stdout[-1500:]!r}  stderr tail: {e.stderr[-3000:]!r}")


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(script, world, env=None, timeout=600):
    """tests/<script> on `world` ranks under torch.distributed.run -> CompletedProcess."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "tests", script)]
    return run_job_or_fail(cmd, env, timeout)


def bench_line(args, tmp_path, name, env=None):
    """Run `bench.py --full` in a child process -> (the short contract line of its stdout, the full report it wrote)."""
    rep = os.path.join(str(tmp_path), name + ".json")
    r = run_job_or_fail([sys.executable, os.path.join(ROOT, "bench.py"), "--full"] + args + ["--report", rep], env, 600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    last = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1]
    assert len(last) < 4096, len(last)            # the contract: a line the driver's 8 KB stdout tail always holds whole
    assert r.stdout.strip().splitlines()[-1] == last
    line = json.loads(last)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "data", "config", "roofline",
                "cpu_baseline"):
        assert key in line, key
    return line, json.load(open(rep))
