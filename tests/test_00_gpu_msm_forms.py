"""GPU: every form of the G2 bucket accumulation gives the oracle's MSM bytes on scalar sets that take its exceptional branches -- a bucket that receives P then P
(doubling), one that receives P, -P and a third point (back to infinity, then set again), a whole group of 127 equal points in one bucket, which the 16-entry segments cut
so that several lanes start with a doubling, and a heavy bucket of 600 entries for the merge kernel (tests/msm_cases.py).  The forms and the switches that select them
for the one-job pass of zkc_msm_debug:
    {}                                          half a wave per bucket (zkc_msm_bucketwave_g2)
    ZKC_G2_BUCKET_WAVE=0                        a lane per segment, the next row held in registers (zkc_msm_accumulate29_g2<1>)
    ZKC_G2_BUCKET_WAVE=0 ZKC_G2_ACC=1 / 2       a lane per segment, the next row fetched through LDS (zkc_msm_accumulate29_g2_dma<1> / <2>)
Section A goes through the G1 accumulation in every configuration.  The switches are read once per process, so each configuration is a child
(tests/host/msm_forms_child.py) with its own time limit, started before this process has initialised the GPU (this file sorts first, like tests/test_00_gpu_switches.py);
after a child that failed no further one is started.  The parent reads the .zkey file, never loads the library, and computes the oracle's MSMs once.

Each child then runs, in the same process and after closing the first key, sections A and B2 of a second key: a generic one of 3 000 wires whose bases are points with
coordinates at the edges of the field (tests/edge_points.py through msm_cases.edge_key) -- Montgomery residues within 64 of q, 0, 1, 2^k, eight all-ones limbs; in B2
twist points outside G2, x.c0 = 0 and x.c1 = 0 among them; equal and opposite bases and infinity throughout -- under scalars of the lowest window only (every addition
takes a window-0 row: the key's own coordinates), uniform ones and the heavy-bucket mix.  The first child writes that key's image into a directory of this module's, the
parent reads it from there."""
import json, os, subprocess, sys
import pytest
import oracle_lib as ol
import msm_cases as mc
import edge_points as ep

pytestmark = pytest.mark.gpu
CONFIGS = [{}, {'ZKC_G2_BUCKET_WAVE': '0'}, {'ZKC_G2_BUCKET_WAVE': '0', 'ZKC_G2_ACC': '1'}, {'ZKC_G2_BUCKET_WAVE': '0', 'ZKC_G2_ACC': '2'}]
_failed = []                                             # the configuration of a child that failed or ran out of time: no further child is started
_ids = lambda c: ','.join('%s=%s' % kv for kv in c.items()) or 'default'


def _child(cfg, edge_dir):
    if _failed:
        pytest.fail('no child started: an earlier one failed under %r' % (_failed[0],))
    env = {k: v for k, v in os.environ.items() if not k.startswith('ZKC_')}
    env.update(cfg)
    try:
        r = subprocess.run([sys.executable, os.path.join(ol.ROOT, 'tests', 'host', 'msm_forms_child.py'), str(edge_dir)], env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _failed.append(cfg)
        raise
    if r.returncode != 0:
        _failed.append(cfg)
    assert r.returncode == 0, (cfg, r.returncode, r.stderr[-1500:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope='module')
def edge_dir(tmp_path_factory):
    return mc.edge_key_dir(tmp_path_factory)


@pytest.fixture(scope='module')
def default_child(edge_dir):
    return _child({}, edge_dir)                           # the first child also makes sure of the keys


@pytest.fixture(scope='module')
def want(default_child, edge_dir):
    from zkcensus_amd import setup
    zk = open(setup.artifact_paths(mc.FORMS_NL)[1], 'rb').read()
    z = ol.zkey_parse(zk)                                 # (points into zk)
    out = {}
    for which in mc.FORMS_SECTIONS:
        std, sets = mc.forms_scalars(z, which)
        msm = ol.msm_g2 if which == 2 else ol.msm_g1
        out[str(which)] = [b.hex() for b in ol.pmap(lambda scb: msm(std, scb), sets)]
    ezk = open(os.path.join(str(edge_dir), mc.EDGE_KEY_FILE), 'rb').read()       # the default child wrote it
    ez = ol.zkey_parse(ezk)
    pools = {64: {ep.g1_std(e.point) for e in ep.g1_pool()} | {bytes(64)}, 128: {ep.g2_std(e.point) for e in ep.g2_pool()} | {bytes(128)}}
    for which in mc.FORMS_SECTIONS:
        std, sets = mc.edge_forms_scalars(ez, which)
        psz = mc.SECTIONS[which][1]
        assert len(std) == psz * 3000 and all(std[i:i + psz] in pools[psz] for i in range(0, len(std), psz)), 'section %d of the edge key holds other points than the pools' % which
        msm = ol.msm_g2 if which == 2 else ol.msm_g1
        out['edge%d' % which] = [b.hex() for b in ol.pmap(lambda scb: msm(std, scb), sets)]
    return out


@pytest.mark.parametrize('cfg', CONFIGS, ids=_ids)
def test_every_g2_form_matches_the_oracle(default_child, want, edge_dir, cfg):
    got = default_child if not cfg else _child(cfg, edge_dir)
    assert set(got) == set(want) == {'0', '2', 'edge0', 'edge2'}
    for which in want:
        bad = [i for i, (g, w) in enumerate(zip(got[which], want[which])) if g != w]
        assert len(got[which]) == len(want[which]) and not bad, (cfg, 'section %s: scalar sets whose MSM differs from the oracle' % which, bad)
