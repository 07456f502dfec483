"""TEST INFRASTRUCTURE for phase 1 (include/zkcensus_ptau_contribute.h), shared by tests/test_ptau_contribute_cpu.py and tests/test_gpu_ptau_contribute.py: a .ptau file
taken apart and put together again, the offsets of a section-7 record, the secrets the tests contribute with and the changed chains every verifier must reject.

The second half is a WRITER of section-7 records that shares nothing with the library but the header's description of the format: U(), pubkey(), transcript(),
challenge() and contribution_hash() over hashlib.blake2b and tests/g2_challenge.py, make_record() and make_chain() over the oracle's scalar multiplications; and
forgeries(), one changed chain per check of zkc_ptau_verify_contributions, each valid under every check before its own."""
import hashlib, struct
import oracle_lib as ol
import ptau_lib as pl
import g2_py
import edge_points as ep
from g2_challenge import challenge_py

R = ol.R
REC = 1288                                    # the fixed part of a record: five points, three proofs of knowledge, transcript, type, paramsLen
OFF_TAU_G1, OFF_POK, OFF_TRANSCRIPT = 0, 448, 1216
OFF_G1_SX, OFF_G2_SPX = 64, 128               # inside a proof of knowledge (256 bytes: g1_s g1_sx g2_spx)

# (tau', alpha', beta') of the chains: full-width, fixed
S1 = (0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100a1b2 % R, 0x0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef % R, 977)
S2 = (3, 0x2b7e151628aed2a6abf7158809cf4f3c2b7e151628aed2a6abf7158809cf4f3c % R, R - 5)
S3 = (R - 2, 12345678901234567890, 0x30000000000000000000000000000000000000000000000000000000deadbeef % R)


def read_sections(path):
    """-> (id -> bytearray of the body, the ids in file order)"""
    z = open(path, 'rb').read()
    assert z[:4] == b'ptau'
    out, order, p = {}, [], 12
    for _ in range(struct.unpack_from('<I', z, 8)[0]):
        i, sz = struct.unpack_from('<IQ', z, p)
        out[i] = bytearray(z[p + 12:p + 12 + sz]); order.append(i); p += 12 + sz
    assert p == len(z)
    return out, order


def write_sections(path, secs, order=None):
    with open(path, 'wb') as f:
        f.write(pl.assemble(secs, order))
    return str(path)


def records(sec7):
    """the records of a section-7 body as (offset, length) pairs"""
    n, at, out = struct.unpack_from('<I', sec7, 0)[0], 4, []
    for _ in range(n):
        plen = struct.unpack_from('<I', sec7, at + REC - 4)[0]
        out.append((at, REC + plen)); at += REC + plen
    assert at == len(sec7)
    return out


def product(secrets):
    t = a = b = 1
    for s in secrets:
        t, a, b = t * s[0] % R, a * s[1] % R, b * s[2] % R
    return t, a, b


def rejects(power=3):
    """name -> (change(secs of the LAST file of a chain of three), the words its reason must hold).  Each changes section 7 or a point section of a valid chain's last file."""
    def flip(off_in_record, rec):
        def change(secs):
            at, _ = records(secs[7])[rec]
            secs[7][at + off_in_record] ^= 1
        return change

    def other_tau(secs):                       # record 2's tauG1 becomes another point of the curve: 5 G
        at, _ = records(secs[7])[2]
        secs[7][at + OFF_TAU_G1:at + OFF_TAU_G1 + 64] = pl.g1_mont(5)

    def last_points(secs):                     # section 4's first point is what record 2 calls alphaG1: another point there
        secs[4][0:64] = pl.g1_mont(9)

    def swap(secs):                            # T_3 and T_4: no record names them, the sums of zkc_ptau_verify see them
        a, b = bytes(secs[2][3 * 64:4 * 64]), bytes(secs[2][4 * 64:5 * 64])
        secs[2][3 * 64:4 * 64], secs[2][4 * 64:5 * 64] = b, a

    def drop_middle(secs):
        rs = records(secs[7])
        at, ln = rs[1]
        secs[7][:] = struct.pack('<I', 2) + bytes(secs[7][4:at]) + bytes(secs[7][at + ln:])

    return {
        'g1_sx': (flip(OFF_POK + 256 + OFF_G1_SX + 3, 2), ['contribution 2', 'g1_sx of alpha']),
        'g2_spx': (flip(OFF_POK + 512 + OFF_G2_SPX + 70, 2), ['contribution 2', 'g2_spx of beta']),
        'transcript': (flip(OFF_TRANSCRIPT + 9, 2), ['contribution 2', 'the stored transcript is not the recomputed one']),
        'tauG1': (other_tau, ['contribution 2', 'the chain step of tau fails']),
        'last_points': (last_points, ["check 4: the last contribution's points are not the next file's"]),
        'swap': (swap, ['check 5', 'section 2 is not the powers of one tau']),
        'drop_middle': (drop_middle, ['contribution 1', 'the stored transcript is not the recomputed one']),
    }


# ================ section 7 restated: include/zkcensus_ptau_contribute.h, "Section 7 as this library writes it" ================
Q = ol.Q
MONT_INV = pow(1 << 256, -1, Q)
FIVE = (('tauG1', 0, 64), ('tauG2', 64, 128), ('alphaG1', 192, 64), ('betaG1', 256, 64), ('betaG2', 320, 128))       # name, offset in the record, width
KEYS = ('tau', 'alpha', 'beta')
S4 = (0x0f1e2d3c4b5a69788796a5b4c3d2e1f00f1e2d3c4b5a69788796a5b4c3d2e1f0 % R, 31337, R - 977)                     # secrets no chain of the tests holds
GEN_FIVE = tuple(pl.to_mont(g) for g in (pl.G1_GEN, pl.G2_GEN, pl.G1_GEN, pl.G1_GEN, pl.G2_GEN))                       # what a chain starts from without a previous file


def from_mont(b):
    return b''.join((int.from_bytes(b[i:i + 32], 'little') * MONT_INV % Q).to_bytes(32, 'little') for i in range(0, len(b), 32))


def U(pt_mont):
    """a point of the file as a hash takes it: big-endian standard-form x || y, in G2 c1 before c0; infinity is zeros with bit 0x40 of the first byte"""
    s = from_mont(pt_mont)
    if not any(s):
        return bytes([0x40]) + bytes(len(s) - 1)
    c = [s[i:i + 32][::-1] for i in range(0, len(s), 32)]
    if len(c) == 4: c = [c[1], c[0], c[3], c[2]]
    return b''.join(c)


def five_of(rec):
    return tuple(bytes(rec[o:o + w]) for _, o, w in FIVE)


def poks_of(rec):
    """[(g1_s, g1_sx, g2_spx)] for tau, alpha, beta"""
    return [tuple(bytes(rec[OFF_POK + 256 * i + o:OFF_POK + 256 * i + o + w]) for o, w in ((0, 64), (OFF_G1_SX, 64), (OFF_G2_SPX, 128))) for i in range(3)]


def pubkey(rec):
    out = b''.join(U(p) for p in five_of(rec)) + b''.join(U(p) for k in poks_of(rec) for p in k) + bytes(rec[OFF_TRANSCRIPT:OFF_TRANSCRIPT + 64])
    assert len(out) == 1280
    return out


def _prefix(power, recs):
    return b'zkc-ptau' + struct.pack('<I', power) + b''.join(pubkey(r) for r in recs)


def transcript(power, earlier, poks):
    """of the record that follows the records `earlier` and holds the proofs of knowledge poks = [(g1_s, g1_sx, ..)] for tau, alpha, beta"""
    return hashlib.blake2b(_prefix(power, earlier) + b''.join(U(k[0]) + U(k[1]) for k in poks), digest_size=64).digest()


def contribution_hash(power, recs):
    return hashlib.blake2b(_prefix(power, recs), digest_size=64).digest()


def challenge(tr, i):
    """g2_sp of key i (0 tau, 1 alpha, 2 beta) under the transcript tr, 128 B standard form"""
    return g2_py.g2_bytes(challenge_py(hashlib.blake2b(tr + bytes([i]), digest_size=64).digest()))


def _mul(pt_mont, k):
    """k * a point of the file, Montgomery form in and out, by the oracle"""
    std = from_mont(pt_mont)
    return pl.to_mont(ol.g1_mul(std, k) if len(std) == 64 else ol.msm_g2(std, ol.le32(k)))


def default_pok_scalars(k):
    return [int.from_bytes(hashlib.sha256(b'pok scalar %d %d' % (k, i)).digest(), 'little') % R or 1 for i in range(3)]


def make_record(power, earlier_records, before_five, secrets, name='', pok_scalars=None):
    """the record of a contribution of secrets = (tau', alpha', beta') to a file whose five points were before_five (Montgomery bytes, in the record's order) and whose
    records were earlier_records; g1_s of key i = pok_scalars[i] G"""
    pok_scalars = pok_scalars or default_pok_scalars(len(earlier_records))
    x = (secrets[0], secrets[0], secrets[1], secrets[2], secrets[2])
    five = [_mul(p, k) for p, k in zip(before_five, x)]
    g1 = [pl.g1_mont(s) for s in pok_scalars]
    poks = [(g1[i], _mul(g1[i], secrets[i])) for i in range(3)]
    tr = transcript(power, earlier_records, poks)
    body = b''.join(five) + b''.join(poks[i][0] + poks[i][1] + pl.to_mont(ol.msm_g2(challenge(tr, i), ol.le32(secrets[i]))) for i in range(3)) + tr
    nm = name.encode()[:64]
    params = bytes([1, len(nm)]) + nm if nm else b''
    rec = body + struct.pack('<II', 0, len(params)) + params
    assert len(rec) == REC + len(params)
    return rec


def section7(recs):
    return bytearray(struct.pack('<I', len(recs)) + b''.join(recs))


def make_chain(power, secrets_list, names=None):
    """-> (sections 1 .. 7 of the file after the contributions secrets_list to a new file, its records): sections 2 .. 6 from ptau_lib at the product of the secrets"""
    recs, five = [], GEN_FIVE
    for k, s in enumerate(secrets_list):
        recs.append(make_record(power, recs, five, s, names[k] if names else 'py%d' % k))
        five = five_of(recs[-1])
    secs = pl.sections(power, *product(secrets_list))
    out = {i: secs[i] for i in range(1, 7)}
    out[7] = section7(recs)
    return out, recs


def outside_g2_mont():
    """a point of the twist outside G2 from the field-edge pool, as the file stores it"""
    return ep.g2_mont(next(e.point for e in ep.g2_pool() if not e.in_g2))


def forgeries(power, secrets_list):
    """name -> (change_next, change_prev, words): the last file of make_chain(power, secrets_list) (three contributions) changed so that exactly the named check of
    zkc_ptau_verify_contributions refuses it.  change_next(secs) edits that file's sections.  change_prev is None for a chain from the generators; otherwise the previous
    file is the one after the FIRST contribution, edited by change_prev(secs).  words: what the reason must hold -- the contribution's number and the check's own text.
    Every forgery sits in the last record (index 2) or in the file's points, so that no transcript of a later record moves, and is valid under every earlier check:
    a record's own transcript hashes neither its five points nor its g2_spx."""
    last = len(secrets_list) - 1
    who = 'contribution %d' % last

    def rec_at(secs):
        return records(secs[7])[last][0]

    def put(off, value):                          # value: bytes, or a function that gives them (the twist pool is made when a forgery is first applied)
        def change(secs):
            at, v = rec_at(secs), value() if callable(value) else value
            secs[7][at + off:at + off + len(v)] = v
        return change

    def other_secret(i):                          # g2_spx of key i = x' g2_sp, x' = x + 1: a point of G2, and the transcript stays
        def change(secs):
            at = rec_at(secs)
            tr = bytes(secs[7][at + OFF_TRANSCRIPT:at + OFF_TRANSCRIPT + 64])
            o = at + OFF_POK + 256 * i + OFF_G2_SPX
            secs[7][o:o + 128] = pl.to_mont(ol.msm_g2(challenge(tr, i), ol.le32((secrets_list[last][i] + 1) % R or 2)))
        return change

    def both(*changes):
        def change(secs):
            for c in changes: c(secs)
        return change

    def file_point(sec, idx, value):
        def change(secs):
            v = value() if callable(value) else value
            secs[sec][idx * len(v):(idx + 1) * len(v)] = v
        return change

    def resign(k):                                # record k made again, completely and validly, under S4; the later records and the sections stay
        def change(secs):
            rs = [bytes(secs[7][a:a + n]) for a, n in records(secs[7])]
            before = five_of(rs[k - 1]) if k else GEN_FIVE
            rs[k] = make_record(power, rs[:k], before, S4, 'resigned')
            secs[7][:] = section7(rs)
        return change

    off5 = {n: o for n, o, _ in FIVE}
    spx = lambda i: OFF_POK + 256 * i + OFF_G2_SPX
    pok_fails = lambda i: [who, 'the proof of knowledge of %s fails: sameRatio(g1_s, g1_sx; g2_sp, g2_spx)' % KEYS[i]]
    check4 = ["check 4: the last contribution's points are not the next file's"]
    out = {
        '3.1 tauG2 outside G2': (put(off5['tauG2'], outside_g2_mont), None, [who, 'tauG2 is at infinity or not in G2']),
        '3.1 g2_spx of alpha outside G2': (put(spx(1), outside_g2_mont), None, [who, 'g2_spx of alpha is at infinity or not in G2']),
        '3.1 betaG1 at infinity': (put(off5['betaG1'], bytes(64)), None, [who, 'betaG1 is at infinity or not on the curve']),
        '3.4 alphaG1 another multiple': (put(off5['alphaG1'], pl.g1_mont(11)), None, [who, 'the chain step of alpha fails: sameRatio(alphaG1 before, after; g2_sp, g2_spx)']),
        '3.4 betaG1 another multiple': (put(off5['betaG1'], pl.g1_mont(11)), None, [who, 'the chain step of beta fails: sameRatio(betaG1 before, after; g2_sp, g2_spx)']),
        '3.5 tauG2 is 5 G2': (put(off5['tauG2'], pl.g2_mont(5)), None, [who, 'tauG1 and tauG2 hold different tau: sameRatio(G1, tauG1; G2, tauG2) fails']),
        '3.5 betaG2 is 5 G2': (put(off5['betaG2'], pl.g2_mont(5)), None, [who, 'betaG1 and betaG2 hold different beta: sameRatio(G1, betaG1; G2, betaG2) fails']),
        '4 section 2 point 1': (file_point(2, 1, pl.g1_mont(9)), None, check4),
        '4 section 3 point 1': (file_point(3, 1, pl.g2_mont(9)), None, check4),
        '4 section 5 point 0': (file_point(5, 0, pl.g1_mont(9)), None, check4),
        '4 section 6': (file_point(6, 0, pl.g2_mont(9)), None, check4),
        '4 re-signed tail': (resign(last), None, check4),
        '3.2 re-signed middle': (resign(last - 1), None, [who, 'the stored transcript is not the recomputed one']),
        '3.3 before 3.5: two defects': (both(other_secret(0), put(off5['betaG2'], pl.g2_mont(5))), None, pok_fails(0)),
        '3 the chain starts outside G2': (lambda secs: None, file_point(3, 1, outside_g2_mont),
                                          ["check 3: a point the chain starts from (the previous file's tauG1[1], tauG2[1], alphaTauG1[0], betaTauG1[0], betaG2) is not in its group"]),
    }
    for i in range(3):
        out['3.3 g2_spx of %s under another secret' % KEYS[i]] = (other_secret(i), None, pok_fails(i))
    return out
