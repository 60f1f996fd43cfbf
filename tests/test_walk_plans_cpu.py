"""No GPU: everything the host-side planning code decides -- parameter tables, arena sizes, workspace sizes of the U-Net (inference, fp8,
run cache, training) and the VAE -- as scripts/walk_plans.py prints it, against the recorded text of profiles/walk_common_plans.txt.  A
host-only change of the walks leaves every byte count what it was.  One child process (the library reads its switches once per process)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_plans_equal_the_recorded_text():
    env = {k: v for k, v in os.environ.items() if not k.startswith("DFH_")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "walk_plans.py")], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recorded = [l for l in open(os.path.join(ROOT, "profiles", "walk_common_plans.txt")).read().splitlines() if not l.startswith("#")]
    printed = r.stdout.splitlines()
    assert len(printed) == len(recorded) > 3000
    differ = [(i, a, b) for i, (a, b) in enumerate(zip(printed, recorded)) if a != b]
    assert not differ, f"{len(differ)} lines differ from profiles/walk_common_plans.txt, the first: {differ[0]}"
