"""TEST INFRASTRUCTURE for phase 1 (include/zkcensus_ptau_contribute.h), shared by tests/test_ptau_contribute_cpu.py and tests/test_gpu_ptau_contribute.py: a .ptau file
taken apart and put together again, the offsets of a section-7 record, the secrets the tests contribute with and the changed chains every verifier must reject."""
import struct
import oracle_lib as ol
import ptau_lib as pl

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
