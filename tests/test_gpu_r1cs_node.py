"""GPU, Node: snarkjs' wtns.check(r1csFile, wtnsFile, logger) through the N-API addon (napi/index.js, zkc_r1cs_load / zkc_r1cs_check).  The witness comes from the CPU oracle
and the .wtns image from the host-only writer, so this process starts node without having touched the GPU itself; the expected index is Python's (r1cs.R1CS.check)."""
import ctypes, json, os, random, shutil, subprocess, sys
import pytest
import oracle_lib as ol
from zkcensus_amd import r1cs, _native

pytestmark = pytest.mark.gpu


def test_node_wtns_check(tmp_path):
    node = shutil.which('node')
    if not node or not os.path.exists(os.path.join(ol.ROOT, 'napi', 'zkcensus.node')):
        pytest.skip('node or the built addon is not available on this box')
    sys.path.insert(0, os.path.join(ol.ROOT, 'tools'))
    from census_gen import random_voter
    lib = _native.load()
    L, cs = r1cs.build(10)
    r1 = str(tmp_path / 'census10.r1cs'); cs.write(r1)
    rc, w = ol.witness(random_voter(random.Random(3), ol.poseidon, nLevels=10, depth_c=7, depth_s=2), nLevels=10)
    assert rc == 0
    wit = [int.from_bytes(w[32 * i:32 * i + 32], 'little') for i in range(L.nWires)]
    assert cs.check(wit) == -1
    bad = list(wit); bad[L.off_sik + 9] = (bad[L.off_sik + 9] + 1) % r1cs.R
    want = cs.check(bad)
    n_bad = sum(1 for a, b, c in cs.cons if (r1cs.lc_eval(a, bad) * r1cs.lc_eval(b, bad) - r1cs.lc_eval(c, bad)) % r1cs.R)
    assert want >= 0 and n_bad >= 1
    def wtns_file(name, payload):
        need = lib.zkc_wtns_write(payload, L.nWires, None, 0)
        out = ctypes.create_string_buffer(need)
        lib.zkc_wtns_write(payload, L.nWires, out, need)
        p = str(tmp_path / name); open(p, 'wb').write(out.raw)
        return p
    good_p, bad_p = wtns_file('good.wtns', w), wtns_file('bad.wtns', b''.join(x.to_bytes(32, 'little') for x in bad))
    js = ("const z=require('./napi'),fs=require('fs');const [r1,g,b]=process.argv.slice(-3);(async()=>{"
          "const log=[];const logger={info:m=>log.push(['info',m]),warn:m=>log.push(['warn',m])};"
          "const a=await z.wtns.check(r1,g,logger);const c=await z.wtns.check(fs.readFileSync(r1),{type:'mem',data:fs.readFileSync(b)},logger);"
          "const d=await z.wtns.check(r1,b);console.log(JSON.stringify({a,c,d,log}))})().catch(e=>{console.error(e);process.exit(1)})")
    try:
        r = subprocess.run([node, '-e', js, r1, good_p, bad_p], cwd=ol.ROOT, capture_output=True, text=True, timeout=300)
    except OSError as e:                                   # the box refused to start a child program from this process
        pytest.skip('cannot start node from this process: %s' % e)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j['a'] is True and j['c'] is False and j['d'] is False
    assert j['log'][0][0] == 'info'
    kind, msg = j['log'][1]
    assert kind == 'warn' and 'constraint %d ' % want in msg and '(%d violated' % n_bad in msg, msg
