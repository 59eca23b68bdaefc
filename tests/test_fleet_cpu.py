"""CPU tests of the fleet (per-row airframes): the host logic under sanitizers, the expected-value construction of the GPU suite
(that it separates the classes at all), and the Python refusals that need no device."""
import os
import subprocess

import numpy as np
import pytest

from tests import fleet_spec as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fleet_host_logic_under_sanitizers(tmp_path):
    """tests/fleet_host_main.cpp, g++ -fsanitize=address,undefined: the table builder of np_f16_host.h — K records equal K separate results byte
    for byte, K = 0 and K = 65 537 refused, a non-finite mass in class 2 refused by class number — and the refusals a fleet context answers with"""
    exe = tmp_path / 'fleet_host_main'
    subprocess.run(['g++', '-std=c++17', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', str(exe),
                    os.path.join(ROOT, 'tests', 'fleet_host_main.cpp')], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, f'exit status {r.returncode}:\n{r.stderr[-4000:]}'
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr
    ok = [ln[3:] for ln in r.stdout.splitlines() if ln.startswith('ok ')]
    for what in ('K records equal K separate results byte for byte', 'K = 0 is refused', 'K = 65537 is refused',
                 'a non-finite mass in class 2 is refused by class number', 'K = 65536 is accepted'):
        assert what in ok, (what, ok)
    msg = [ln for ln in r.stdout.splitlines() if ln.startswith('message ')]
    assert msg and 'class 2' in msg[0] and 'fleet' in msg[0]


def test_row_selection_separates_the_classes():
    """The expected value of the GPU suite is three oracle runs with rows picked by class.  That proves something only if the classes fly apart:
    after 40 free-running steps at N = 293, every pair of per-class runs differs in state bits on at least 90 % of the rows — a condition on the
    overrides chosen in tests/fleet_spec.py, checked for every task and both solvers the GPU suite runs."""
    for task in ('heading', 'control', 'tracking'):
        for solver in (None, 'rk4'):
            runs = [fs.class_run(task, solver, c) for c in fs.CLASSES]
            for a in range(3):
                for b in range(a + 1, 3):
                    frac = float(fs.state_bits_differ(runs[a][fs.STEPS][0]['s'], runs[b][fs.STEPS][0]['s']).mean())
                    print(f'{task}/{solver or "euler"}: classes {a} and {b} differ on {100 * frac:.1f} % of the rows at step {fs.STEPS}')
                    assert frac >= 0.9, (task, solver, a, b, frac)
    # ... and the selection really picks: the mixed batch equals none of the single-class runs, and each of its rows equals its class's row
    idx = fs.mixed_index()
    out, resets = fs.expected_run('heading', None, fs.CLASSES, idx)
    runs = [fs.class_run('heading', None, c) for c in fs.CLASSES]
    s = out[fs.STEPS][0]['s']
    for c in range(3):
        assert fs.same(s[idx == c], runs[c][fs.STEPS][0]['s'][idx == c])
        assert not fs.same(s, runs[c][fs.STEPS][0]['s'])
    assert all(r >= 1 for r in resets), resets
    assert sorted(set(idx.tolist())) == [0, 1, 2] and (idx[192:256] == 1).all() and (idx[256:288] == 2).all()
    for w in range(3):                                   # the first three waves hold every class
        assert set(idx[64 * w:64 * (w + 1)].tolist()) == {0, 1, 2}


def test_python_refusals_need_no_device(tmp_path):
    from neuralplane_amd.core import F16Batch, fleet_classes
    from neuralplane_amd.envs.control_env import ControlEnv
    from neuralplane_amd.envs.planning_env import PlanningEnv
    from neuralplane_amd.envs.utils.utils import parse_config
    with pytest.raises(ValueError, match='airframes'):
        ControlEnv(num_envs=4, config='heading', model='F16', random_seed=0, device='cuda:0', airframes=[{}, {'mass': 700}], airframe={'mass': 700})
    with pytest.raises(ValueError, match='airframes'):
        ControlEnv(num_envs=4, config='heading', model='F16', random_seed=0, device='cuda:0', airframes=[])
    with pytest.raises(ValueError, match='airframes'):
        PlanningEnv(num_envs=4, config='tracking', model='F16', random_seed=0, device='cuda:0', controller=lambda *a, **k: None, airframes=[])
    with pytest.raises(ValueError, match=r'airframes\[1\].*wingspan'):
        ControlEnv(num_envs=4, config='heading', model='F16', random_seed=0, device='cuda:0', airframes=[{}, {'wingspan': 30.0}])
    with pytest.raises(ValueError, match='airframes'):
        ControlEnv(num_envs=4, config='heading', model='F16', random_seed=0, device='cuda:0', airframes={'mass': 700})   # a mapping is one class, not a list
    with pytest.raises(ValueError, match='airframe_index'):
        F16Batch(4, parse_config('heading'), 'heading', 'cuda:0', airframe_index=np.zeros(4, np.int32))                 # an index without classes
    from neuralplane_amd.envs.singlecombat_env import SingleCombatEnv
    with pytest.raises(ValueError, match='fleet'):                                                                      # SingleCombat: refused by name
        SingleCombatEnv(num_envs=2, config='selfplay', random_seed=0, device='cuda:0', airframes=[{}, {'mass': 700}])
    with pytest.raises(ValueError, match='fleet'):
        SingleCombatEnv(num_envs=2, config='selfplay', random_seed=0, device='cuda:0', airframe_index=np.zeros(4, np.int32))
    # the YAML key `airframes:` — a scenario file with an unknown field in its second class
    text = open(os.path.join(ROOT, 'neuralplane_amd', 'envs', 'configs', 'heading.yaml')).read()
    (tmp_path / 'fleet_bad.yaml').write_text(text + '\nairframes:\n  - {}\n  - {mass: 700, wingspan: 30.0}\n')
    with pytest.raises(ValueError, match=r'airframes\[1\].*wingspan'):
        F16Batch(4, parse_config(str(tmp_path / 'fleet_bad')), 'heading', 'cuda:0')
    sp = open(os.path.join(ROOT, 'neuralplane_amd', 'envs', 'configs', 'selfplay.yaml')).read()
    (tmp_path / 'combat_fleet.yaml').write_text(sp + '\nairframes:\n  - {}\n  - {mass: 700}\n')
    with pytest.raises(ValueError, match='fleet'):
        SingleCombatEnv(num_envs=2, config=str(tmp_path / 'combat_fleet'), random_seed=0, device='cuda:0')
    (tmp_path / 'fleet_both.yaml').write_text(text + '\nairframe: {mass: 700}\nairframes:\n  - {}\n')
    with pytest.raises(ValueError, match='exclude'):
        F16Batch(4, parse_config(str(tmp_path / 'fleet_both')), 'heading', 'cuda:0')
    # what is accepted: the blocks are those of `airframe=`, {} the all-zero block
    (tmp_path / 'fleet_ok.yaml').write_text(text + '\nairframes:\n  - {}\n  - {mass: 700, Jy: 60000}\n')
    from neuralplane_amd import _lib
    arr = fleet_classes(parse_config(str(tmp_path / 'fleet_ok')))
    assert len(arr) == 2 and not any(bytes(arr[0])) and bytes(arr[1]) == bytes(_lib.airframe({'mass': 700, 'Jy': 60000}))
    assert fleet_classes(parse_config('heading')) is None
