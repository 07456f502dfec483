"""GPU: every form of the G2 bucket accumulation gives the oracle's MSM bytes on scalar sets that take its exceptional branches -- a bucket that receives P then P
(doubling), one that receives P, -P and a third point (back to infinity, then set again), a whole group of 127 equal points in one bucket, which the 16-entry segments cut
so that several lanes start with a doubling, and a heavy bucket of 600 entries for the merge kernel (tests/msm_cases.py).  The forms and the switches that select them
for the one-job pass of zkc_msm_debug:
    {}                                          half a wave per bucket (zkc_msm_bucketwave_g2)
    ZKC_G2_BUCKET_WAVE=0                        a lane per segment, the next row held in registers (zkc_msm_accumulate29_g2<1>)
    ZKC_G2_BUCKET_WAVE=0 ZKC_G2_ACC=1 / 2       a lane per segment, the next row fetched through LDS (zkc_msm_accumulate29_g2_dma<1> / <2>)
Section A goes through the G1 accumulation in every configuration.  The switches are read once per process, so each configuration is a child
(tests/host/msm_forms_child.py) with its own time limit, started before this process has initialised the GPU (this file sorts first, like tests/test_00_gpu_switches.py);
after a child that failed no further one is started.  The parent reads the .zkey file, never loads the library, and computes the oracle's MSMs once."""
import json, os, subprocess, sys
import pytest
import oracle_lib as ol
import msm_cases as mc

pytestmark = pytest.mark.gpu
CONFIGS = [{}, {'ZKC_G2_BUCKET_WAVE': '0'}, {'ZKC_G2_BUCKET_WAVE': '0', 'ZKC_G2_ACC': '1'}, {'ZKC_G2_BUCKET_WAVE': '0', 'ZKC_G2_ACC': '2'}]
_failed = []                                             # the configuration of a child that failed or ran out of time: no further child is started
_ids = lambda c: ','.join('%s=%s' % kv for kv in c.items()) or 'default'


def _child(cfg):
    if _failed:
        pytest.fail('no child started: an earlier one failed under %r' % (_failed[0],))
    env = {k: v for k, v in os.environ.items() if not k.startswith('ZKC_')}
    env.update(cfg)
    try:
        r = subprocess.run([sys.executable, os.path.join(ol.ROOT, 'tests', 'host', 'msm_forms_child.py')], env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _failed.append(cfg)
        raise
    if r.returncode != 0:
        _failed.append(cfg)
    assert r.returncode == 0, (cfg, r.returncode, r.stderr[-1500:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope='module')
def default_child():
    return _child({})                                     # the first child also makes sure of the key


@pytest.fixture(scope='module')
def want(default_child):
    from zkcensus_amd import setup
    zk = open(setup.artifact_paths(mc.FORMS_NL)[1], 'rb').read()
    z = ol.zkey_parse(zk)                                 # (points into zk)
    out = {}
    for which in mc.FORMS_SECTIONS:
        std, sets = mc.forms_scalars(z, which)
        msm = ol.msm_g2 if which == 2 else ol.msm_g1
        out[str(which)] = [b.hex() for b in ol.pmap(lambda scb: msm(std, scb), sets)]
    return out


@pytest.mark.parametrize('cfg', CONFIGS, ids=_ids)
def test_every_g2_form_matches_the_oracle(default_child, want, cfg):
    got = default_child if not cfg else _child(cfg)
    assert set(got) == set(want)
    for which in want:
        bad = [i for i, (g, w) in enumerate(zip(got[which], want[which])) if g != w]
        assert len(got[which]) == len(want[which]) and not bad, (cfg, 'section %s: scalar sets whose MSM differs from the oracle' % which, bad)
