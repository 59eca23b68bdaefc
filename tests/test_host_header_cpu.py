"""CPU tests of the host-only logic behind the C ABI (neuralplane_amd/csrc/np_f16_host.h): tests/host_logic_main.cpp built with g++ under the
address and undefined-behaviour sanitizers — no hipcc, no library loaded into python.  One run of the program packs the shipped weights asset
into the three record layouts, offers the packer cut and corrupted copies of it, and prints the constants the kernels get; the tests rebuild all
of that in numpy from the layout comments of np_nets.h and the rounding rules of the reference, and compare bit patterns."""
import os
import re
import struct
import subprocess
import sys
import types

import numpy as np
import pytest

from test_gemm_order_cpu import _asset_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, 'tools')
CSRC = os.path.join(ROOT, 'neuralplane_amd', 'csrc')
ACT_SHIFT = 40
f32 = np.float32


def _tools():
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import emulate_dual_asm
    import emulate_gemm_asm
    import gen_mlp_asm
    return gen_mlp_asm, emulate_gemm_asm, emulate_dual_asm


def _blob():
    from neuralplane_amd.core import ASSET_BLOB
    return open(ASSET_BLOB, 'rb').read()


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    """the program's one run: (stdout lines as {name: value text}, stderr, directory with the layout files, the two cfg records)"""
    from neuralplane_amd.core import ASSET_BLOB, cfg_from_config, combat_cfg_from_config
    from neuralplane_amd.envs.utils.utils import parse_config
    d = tmp_path_factory.mktemp('host_logic')
    exe = d / 'host_logic_main'
    subprocess.run(['g++', '-std=c++17', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', str(exe),
                    os.path.join(ROOT, 'tests', 'host_logic_main.cpp')], check=True)
    cfg, ccfg = cfg_from_config(parse_config('heading'), 'heading'), combat_cfg_from_config(parse_config('selfplay'))
    (d / 'cfg.bin').write_bytes(bytes(cfg))
    (d / 'combat_cfg.bin').write_bytes(bytes(ccfg))
    r = subprocess.run([str(exe), ASSET_BLOB, str(d), str(d / 'cfg.bin'), str(d / 'combat_cfg.bin')], capture_output=True, text=True)
    print(r.stderr)
    assert r.returncode == 0, f'exit status {r.returncode} (a sanitizer report or an accepted hostile blob):\n{r.stderr[-4000:]}'
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr
    values = dict(line.split(' ') for line in r.stdout.splitlines())
    return types.SimpleNamespace(values=values, stderr=r.stderr, dir=d, cfg=cfg, ccfg=ccfg)


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------
def _classes():
    """np_nets.h::CLASSES as [(name, (n_in, h1, h2, h3), [group names], [NetId of each member])]"""
    src = open(os.path.join(CSRC, 'np_nets.h')).read()
    ids = [s.strip() for s in re.search(r'enum NetId : int \{(.*?)\};', src, re.S).group(1).split(',')]
    rows = re.findall(r'/\* (CL_\w+)\s*\*/ \{(\d+), (\d+), (\d+), (\d+), \{([^}]*)\}, (\d+), \d+,\s*\{([^}]*)\}\}', src)
    out = []
    for name, n_in, h1, h2, h3, grp, count, nets in rows:
        nets = [ids.index(s.strip()) for s in nets.split(',')]
        assert len(nets) == int(count)
        out.append((name, (int(n_in), int(h1), int(h2), int(h3)), [g.strip() for g in grp.split(',')][:int(n_in)], nets))
    return out


def _scaled_net(blob, net):
    """the net with its parameters scaled as the records carry them: first layer's weights and every hidden bias x 2^-ACT_SHIFT, output
    weights x 2^+ACT_SHIFT -> ([(W[out][in], b[out])], (w[in], b), fp32 out_std, fp32 out_mean)"""
    _, Ws, bs, _, _, out_mean, out_std, _ = _asset_net(blob, net)
    layers = [(np.ldexp(W, -ACT_SHIFT) if l == 0 else W, np.ldexp(b, -ACT_SHIFT)) for l, (W, b) in enumerate(zip(Ws[:-1], bs[:-1]))]
    return layers, (np.ldexp(Ws[-1][0], ACT_SHIFT), bs[-1][0]), f32(out_std), f32(out_mean)


def _pack_first(net, n):
    """one record of the first layout, from the layout comment of np_nets.h: per hidden layer bias[out] then W^T[in][out], every row padded
    to an even length; output layer (bias, 0), W[0][0..in) padded to even; out_std, out_mean; zero padding to n floats"""
    layers, (w, b), sd, mu = net
    rec = []
    for W, bias in layers:
        out, inn = W.shape
        rows = np.zeros((inn + 1, out + (out & 1)), f32)
        rows[0, :out] = bias
        rows[1:, :out] = W.T
        rec += list(rows.ravel())
    rec += [b, f32(0)] + list(w) + [f32(0)] * (len(w) & 1) + [sd, mu]
    assert len(rec) <= n
    return np.array(rec + [0.0] * (n - len(rec)), f32)


def _expected_layouts(blob):
    G, EG, ED = _tools()
    classes = _classes()
    assert [(c[0], c[1], len(c[3])) for c in classes] == [(c[0], c[1], c[3]) for c in G.CLASSES]
    assert sorted(n for c in classes for n in c[3]) == [n for n in range(43) if n != 24]          # all 42 live nets, each once
    kb = np.zeros(G.class_base(len(classes)) + 2 * G.GROUP, f32)
    kbd = np.zeros(G.class_base_nm(len(classes)) + 2 * G.GROUP, f32)
    kbg = np.zeros_like(kb)
    for ci, (_, shape, grps, nets) in enumerate(classes):
        ln, ln_nm = G.record_len(*shape), G.record_len_nm(*shape)
        for m, net in enumerate(nets):
            sn = _scaled_net(blob, net)
            kb[G.class_base(ci) + m * ln:][:ln] = _pack_first(sn, ln)
            kbd[G.class_base_nm(ci) + m * ln_nm:][:ln_nm] = ED.pack_nm(sn, shape)
            _, Ws, bs, in_mean, in_std, out_mean, out_std, mask = _asset_net(blob, net)
            kbg[G.class_base(ci) + m * ln:][:ln] = EG.pack_gemm(list(zip(Ws[:-1], bs[:-1])), (Ws[-1][0], bs[-1][0]), f32(out_std), f32(out_mean), shape)
            # header: (mean, sigma, RN(1 / sigma)) of the group of each input slot; slot k <- k-th set bit of the mask
            for g, k in zip(grps, [k for k in range(3) if mask >> k & 1]):
                sd = f32(in_std[k])
                kb[3 * G.G[g]:3 * G.G[g] + 3] = [f32(in_mean[k]), sd, f32(1.0 / float(sd))]
    kbg[:G.KBLOB_HEADER] = kb[:G.KBLOB_HEADER]
    return kb, kbd, kbg


def _same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_three_record_layouts_of_the_shipped_asset(run):
    blob = _blob()
    kb, kbd, kbg = _expected_layouts(blob)
    for name, want in (('kb', kb), ('kbd', kbd), ('kbg', kbg)):
        got = np.fromfile(run.dir / f'{name}.f32', f32)
        assert _same_bits(got, want), f'{name}: {got.size} floats against {want.size}, first difference at {np.flatnonzero(got.view(np.uint32)[:want.size] != want.view(np.uint32)[:got.size])[:1]}'
    # the PWL tables and their un-normalisation pairs (version-2 blob): the section's floats as they are, (out_std, out_mean) of the table's net
    ver, nn = struct.unpack_from('<II', blob, 8)
    if ver >= 2:
        recs = [struct.unpack_from('<II', blob, 16 + 128 * i + 120) for i in range(nn)]
        q = 16 + 128 * nn + 4 * max(off + n for off, n in recs) + 12
        tables, unnorm = [], []
        for _ in range(22):
            idx = struct.unpack_from('<I', blob, q)[0]
            tables.append(np.frombuffer(blob, f32, 256, q + 8))
            out_mean, out_std = struct.unpack_from('<2d', blob, 16 + 128 * idx + 104)
            unnorm += [f32(out_std), f32(out_mean)]
            q += 8 + 4 * 256
        assert _same_bits(np.fromfile(run.dir / 'pwl.f32', f32), np.concatenate(tables))
        assert _same_bits(np.fromfile(run.dir / 'pwl_unnorm.f32', f32), np.array(unnorm, f32))


def test_the_library_returns_the_same_gemm_records(run):
    from neuralplane_amd import _lib, build
    build.build_hip()
    lib_kbg = np.ctypeslib.as_array(_lib.pack_kblob_gemm(_blob())).copy()
    assert _same_bits(lib_kbg, np.fromfile(run.dir / 'kbg.f32', f32))


# ---- hostile input ---------------------------------------------------------------------------------------------------------------------------
def test_every_cut_or_corrupted_blob_is_refused_with_a_message(run):
    """the program exits 0 only if every case was refused with a non-empty message and no sanitizer spoke (the fixture); here: the cases ran"""
    lines = [l for l in run.stderr.splitlines() if l.strip()]
    assert not any('ACCEPTED' in l for l in lines)
    cuts = [l for l in lines if l.startswith('cut ')]
    assert len(cuts) == 4 + 2 * 43 + 1 + 4                     # 0 / 8 / 15 / 16, the 43 records, the parameter block, the PWL section
    for what in ('n_linear', 'dims[0]', 'dims[1]', 'n_params', 'input_mask', 'param_offset of a class member', 'param_offset of the dead net',
                 'PWL net_index', 'PWL n_segments'):
        assert any(l.startswith(what) for l in lines), what
    assert all('weights blob:' in l for l in lines)           # every message is one of the packer's own


# ---- constants -------------------------------------------------------------------------------------------------------------------------------
# the F-16 literals of the reference (F16_dynamics.py:22-35,61-76,114-116; F16_model.py:52-62)
F16 = dict(g=32.17, mass=636.94, B=30.0, S=300.0, cbar=11.32, xcgr=0.35, xcg=0.30, Heng=0.0, Jy=55814.0, Jxz=982.0, Jz=63100.0, Jx=9496.0,
           ail_ref=21.5, rud_ref=30.0, atm_lapse=0.703e-5, atm_exp=4.14, rho0=2.377e-3, lag_keep=0.9, lag_new=0.1, thrust_frac=0.225,
           thrust_max=76300.0, thrust_unit=0.3048, surf_max=(45.0, 45.0, 45.0))


def _bits(v):
    return '%08x' % int(np.array([v], f32).view(np.uint32)[0])


def _rcp(x):   # RN(1 / c) of the fp32 divisor c, computed in double
    return f32(1.0 / float(f32(x)))


def _expected_airframe(a):
    """every field folded in double first (Python floats), then rounded once to float32"""
    e = {k: f32(a[k]) for k in ('g', 'mass', 'B', 'S', 'cbar', 'Heng', 'Jy', 'Jxz', 'Jz', 'Jx', 'ail_ref', 'rud_ref', 'atm_lapse', 'rho0', 'lag_keep',
                                'lag_new', 'thrust_frac', 'thrust_max', 'thrust_unit')}
    e.update(pad_=f32(0), r_mass=_rcp(a['mass']), r_Jy=_rcp(a['Jy']), r_ail_ref=_rcp(a['ail_ref']), r_rud_ref=_rcp(a['rud_ref']),
             r_thrust_unit=_rcp(a['thrust_unit']))
    e['xc'] = f32(a['xcgr'] - a['xcg'])
    e['cbar_over_B'] = f32(a['cbar'] / a['B'])
    e['c1'] = f32(a['Jz'] * (a['Jz'] - a['Jy']) + a['Jxz'] * a['Jxz'])
    e['c2'] = f32(a['Jxz'] * (a['Jx'] - a['Jy'] + a['Jz']))
    e['c3'] = f32(a['Jz'] - a['Jx'])
    e['c4'] = f32(a['Jx'] * (a['Jx'] - a['Jy']) + a['Jxz'] * a['Jxz'])
    e['denom'] = f32(a['Jx'] * a['Jz'] - a['Jxz'] * a['Jxz'])
    e['r_denom'] = _rcp(e['denom'])
    for k in range(3):
        e[f'surf_max[{k}]'] = f32(a['surf_max'][k])
    out = {k: _bits(v) for k, v in e.items()}
    out['atm_exp'] = '%016x' % int(np.array([float(f32(a['atm_exp']))], np.float64).view(np.uint64)[0])     # (double)(float)4.14
    return out


def _check(values, prefix, want):
    got = {k[len(prefix):]: v for k, v in values.items() if k.startswith(prefix) and '.' not in k[len(prefix):]}
    assert set(got) == set(want), (prefix, set(got) ^ set(want))
    assert got == want, (prefix, {k: (got[k], want[k]) for k in want if got[k] != want[k]})


def test_airframe_constants_round_where_the_reference_rounds(run):
    want = _expected_airframe(F16)
    assert len(want) == 37
    for prefix in ('airframe.', 'devcfg.af.', 'combat.af.'):       # the default block, and the all-zero blocks of the two scenario records
        _check(run.values, prefix, want)


def test_devcfg_constants_round_where_the_reference_rounds(run):
    c = run.cfg
    plain = ('airspeed', 'noise_scale', 'altitude_limit', 'acceleration_limit', 'max_velocity', 'min_velocity', 'min_alpha', 'max_alpha', 'min_beta',
             'max_beta', 'init_T', 'min_altitude', 'min_vt', 'max_heading_increment', 'max_pitch_increment', 'max_velocities_u_increment', 'min_distance')
    want = {k: _bits(getattr(c, k)) for k in plain}
    want.update(dt=_bits(f32(c.dt) - f32(0)), alt_span=_bits(c.max_altitude - c.min_altitude), vt_span=_bits(c.max_vt - c.min_vt),
                dist_span=_bits(c.max_distance - c.min_distance), max_check_interval=str(c.max_check_interval),
                min_check_interval=str(c.min_check_interval), aero_1d_tables=str(int(bool(c.aero_1d_tables))))
    _check(run.values, 'devcfg.', want)


def test_combat_constants_round_where_the_reference_rounds(run):
    c = run.ccfg
    plain = ('airspeed', 'altitude_limit', 'acceleration_limit', 'max_velocity', 'min_velocity', 'min_alpha', 'max_alpha', 'min_beta', 'max_beta',
             'init_T', 'min_altitude', 'min_vt', 'min_heading', 'min_npos', 'min_epos', 'roll_ff', 'gravity')
    want = {k: _bits(getattr(c, k)) for k in plain}
    want.update(dt=_bits(f32(c.dt) - f32(0)), dt_pid=_bits(c.dt), dist_limit_sq=_bits(c.distance_limit ** 2),
                alt_span=_bits(c.max_altitude - c.min_altitude), vt_span=_bits(c.max_vt - c.min_vt), yaw_span=_bits(c.max_heading - c.min_heading),
                npos_span=_bits(c.max_npos - c.min_npos), epos_span=_bits(c.max_epos - c.min_epos),
                scale_min=_bits(min(0.5, 1000.0 / (2.0 * c.airspeed_max))), scale_max=_bits(max(2.0, 1000.0 / (0.7 * c.airspeed_min))),
                max_steps=str(c.max_steps), inner_steps=str(c.inner_steps), aero_1d_tables=str(int(bool(c.aero_1d_tables))))
    _check(run.values, 'combat.', want)
    for axis in ('roll', 'pitch', 'yaw'):
        g = getattr(c, axis)
        pid = {k: _bits(getattr(g, k)) for k in ('Kp', 'Ki', 'Kd', 'Kff', 'Kimax', 'rmax_pos', 'rmax_neg')}
        pid.update(tau=_bits(max(g.tau, 0.05)), ki_on=str(int(g.Ki != 0.0 and c.dt > 0.0)))      # tau's 0.05 floor (rollController.py:44-45)
        _check(run.values, f'combat.{axis}.', pid)
