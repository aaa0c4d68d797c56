"""Cases and CPU references of the particle-world KATs (tests/test_gpu_particles_kat.py), for the
device functions of ggrs_amd/csrc/particles.h: the entity step (advance_entity<Lean>) and the
closed-form Fletcher-16 (fletcher_entity_mod + finish_checksum).  Built with numpy from fixed
seeds; what a case set covers is worked out from the cases themselves, never from a device result.

References: the ship words are oracle.ship_step_batch's, the payload words the recurrence of
particles.h in integers masked to 32 bits (payload_step; payload_step_int is the same in plain
Python ints, and tests/test_particle_kat_cases.py holds both to the oracle's particle world), the
checksum oracle.fletcher16 over the declared byte stream (frame, then the records)."""
import numpy as np

FIELDS = 25            # particles.h kFields: 5 ship words + 20 payload words
PAYLOAD = 20
ENTITY_BYTES = 100
PAYLOAD_MUL = 0x9E3779B1
M32 = 0xFFFFFFFF

FRAMES = (0, 1, 255, 256, 0xFFFF, 0x10000, 0x00FF00FF, 0x01020304, 0x7FFFFFFF)
BIG_N = 160000
BIG_FRAMES = (0x01020304, 0x7FFFFFFF)     # every byte nonzero; the largest counter
CHECKSUM_N = (4, 8, 52, 256, 260, 10000)  # and BIG_N, kept to the constant fills
CONST_FILLS = (0x00, 0x01, 0xFE, 0xFF)


# ---------------------------------------------------------------- the entity step
def payload_step(pay, inputs):
    """p'[k] = p[k] * 0x9E3779B1 + (p[(k + 1) % 20] >> 7) + input on old values, u32 wrap:
    pay [n][20] u32, inputs [n] (the whole byte).  Integers held in u64 (a product of two 32-bit
    values fits) and masked to 32 bits."""
    p = np.ascontiguousarray(pay, np.uint32).astype(np.uint64)
    nxt = np.roll(p, -1, axis=1)  # column k holds p[(k + 1) % 20], column 19 the old p[0]
    inp = np.asarray(inputs, np.uint8).astype(np.uint64)[:, None]
    mask = np.uint64(M32)
    return ((((p * np.uint64(PAYLOAD_MUL)) & mask) + (nxt >> np.uint64(7)) + inp) & mask).astype(np.uint32)


def payload_step_int(row, inp):
    """the same recurrence on one row, in Python integers"""
    old = [int(v) for v in row]
    return [(old[k] * PAYLOAD_MUL + (old[(k + 1) % PAYLOAD] >> 7) + int(inp)) & M32 for k in range(PAYLOAD)]


def special_payload_rows():
    """[rows][20]: all 0; all ones; 0x7f / 0x80 / 0xffffff80 around the >> 7 (each alone, then
    cycled); rows whose p[19] and p[0] differ so that the wrap must read the OLD p[0]"""
    rows = [np.zeros(PAYLOAD, np.uint32), np.full(PAYLOAD, M32, np.uint32)]
    rows += [np.full(PAYLOAD, v, np.uint32) for v in (0x7F, 0x80, 0xFFFFFF80)]
    rows.append(np.array([(0x7F, 0x80, 0xFFFFFF80)[k % 3] for k in range(PAYLOAD)], np.uint32))
    only0 = np.zeros(PAYLOAD, np.uint32)
    only0[0] = 0x80            # p'[19] = (old p[0] >> 7) + input = 1 + input; the new p[0] >> 7 is not 1
    only19 = np.zeros(PAYLOAD, np.uint32)
    only19[19], only19[0] = 0xFFFFFF80, 0x12345680
    rows += [only0, only19, (np.arange(PAYLOAD, dtype=np.uint32) + 1) << np.uint32(7)]
    return np.stack(rows)


def advance_cases(an, order, seed):
    """Lanes of the advance KAT from the step-form cases `order` (indices into an): ship words and
    direction bits of each case with a random high nibble and random payload; then, for every
    special payload row, one lane per input byte 0..255 (ships from the head of `order`).  Returns
    words [n][25] u32 and inputs [n] u8, n no multiple of 64."""
    rng = np.random.default_rng(seed)
    sp = special_payload_rows()
    tail = np.resize(order, sp.shape[0] * 256)
    idx = np.concatenate([order, tail])
    if idx.size % 64 == 0:
        idx = np.concatenate([idx, order[:1]])
    n = idx.size
    words = np.zeros((n, FIELDS), np.uint32)
    words[:, :5] = an["players"][idx]
    words[:, 5:] = rng.integers(0, 1 << 32, (n, PAYLOAD), dtype=np.uint64).astype(np.uint32)
    inputs = (an["inputs"][idx] & 15) | (rng.integers(0, 16, n).astype(np.uint8) << 4)
    t0 = order.size
    words[t0:t0 + tail.size, 5:] = np.repeat(sp, 256, axis=0)
    inputs[t0:t0 + tail.size] = np.tile(np.arange(256, dtype=np.uint8), sp.shape[0])
    return words, inputs.astype(np.uint8)


def advance_reference(oracle, words, inputs):
    want = np.zeros_like(words)
    want[:, :5] = oracle.ship_step_batch(words[:, :5], inputs)
    want[:, 5:] = payload_step(words[:, 5:], inputs)
    return want


# ---------------------------------------------------------------- the checksum
def stream_bytes(frame, words):
    """the declared byte layout of one state: frame (4 bytes LE), then per entity 25 LE words"""
    w = np.ascontiguousarray(words, "<u4").reshape(-1, FIELDS)
    return np.concatenate([np.array([frame], "<u4").view(np.uint8), w.view(np.uint8).ravel()])


def _from_bytes(b, N):
    return np.ascontiguousarray(b, np.uint8).reshape(N, ENTITY_BYTES).view("<u4").astype(np.uint32)


def fill_cases(N, seed):
    """[cases][N][25]: the constant fills, two random states, and two with byte = f(position in the stream)"""
    rng = np.random.default_rng(seed)
    pos = np.arange(ENTITY_BYTES * N, dtype=np.int64) + 4
    out = [np.full((N, FIELDS), c * 0x01010101, np.uint32) for c in CONST_FILLS]
    out += [rng.integers(0, 1 << 32, (N, FIELDS), dtype=np.uint64).astype(np.uint32) for _ in range(2)]
    out += [_from_bytes(((pos * 7 + 3) % 256).astype(np.uint8), N), _from_bytes((255 - pos % 255).astype(np.uint8), N)]
    return np.stack(out)


def single_byte_cases(N=8):
    """[400][N][25]: one nonzero byte (0x01, 0xff) at each of the 100 positions of entity 0 and of entity N - 1"""
    out = np.zeros((2 * 2 * ENTITY_BYTES, N * ENTITY_BYTES), np.uint8)
    i = 0
    for e in (0, N - 1):
        for v in (0x01, 0xFF):
            for j in range(ENTITY_BYTES):
                out[i, e * ENTITY_BYTES + j] = v
                i += 1
    return np.stack([_from_bytes(r, N) for r in out])


def big_cases():
    """[4][160000][25]: the constant fills at the largest entity count (16 MB each)"""
    return np.stack([np.full((BIG_N, FIELDS), c * 0x01010101, np.uint32) for c in CONST_FILLS])


def checksum_sets():
    """(name, N, frames, words [cases][N][25]) of every checksum KAT set but the 160000-entity one"""
    sets = [(f"fills N={N}", N, FRAMES, fill_cases(N, 500 + N)) for N in CHECKSUM_N]
    sets.append(("single bytes N=8", 8, FRAMES, single_byte_cases(8)))
    return sets


def checksum_reference(oracle, N, frames, words):
    """[cases][frames] u16: oracle.fletcher16 of every (state, frame counter) stream"""
    cases = words.shape[0]
    out = np.zeros((cases, len(frames)), np.uint16)
    for j, f in enumerate(frames):
        if N * ENTITY_BYTES <= 1 << 16:  # small streams: the same oracle function, a row per state
            rows = np.stack([stream_bytes(f, words[c]) for c in range(cases)])
            out[:, j] = oracle.fletcher16_batch(rows)
        else:
            for c in range(cases):
                out[c, j] = oracle.fletcher16(stream_bytes(f, words[c]).tobytes())
    return out


def c_e(N):
    """(n - o_e) mod 255 = 100 (N - e) mod 255 of every entity of an N-entity state"""
    return (ENTITY_BYTES * (N - np.arange(N, dtype=np.int64))) % 255


def byte_sum_residues(words):
    """per entity A_e mod 255 of words [..][25]"""
    b = np.ascontiguousarray(words, "<u4").view(np.uint8).reshape(-1, ENTITY_BYTES)
    return b.sum(axis=1, dtype=np.int64) % 255
