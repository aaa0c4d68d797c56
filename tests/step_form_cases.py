"""Cases of the step-form KATs (tests/test_gpu_step_forms.py): player states of ex_game's
State::advance chosen where a restated step can go wrong, each crossed with all 16 direction
inputs, their CPU-oracle results, and the lane orders the device forms are run in.  Also the one
recipe that compiles a device KAT harness.  Everything is built with numpy from fixed seeds; every
value is finite, |v| <= 8 per velocity component, positions in [+0, 600] x [+0, 800] (never -0).

What a case "does" (clamps, mag2, walls, wraps) is worked out from the inputs and the oracle's own
outputs, never from a device result."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

F32 = np.float32
TWO_PI_BITS = 0x40C90FDB           # (float)(2 * pi), box_game.h's kTwoPiBits
ROTATION_SPEED = F32(2.5) / F32(60.0)
FRICTION = F32(0.98)
UP, DOWN, LEFT, RIGHT = 1, 2, 4, 8
CLASS_NAMES = {1: "uniform", 2: "walls", 3: "clamp threshold", 4: "velocity specials", 5: "rotation edges",
               6: "out of domain"}
MAX_PLAYERS_REC = 12               # branch.hip: NS = 8 pipeline stages + 4 trunk players


def compile_kat(name, out_dir):
    """hipcc tests/native/<name>.hip -> out_dir/lib<name>.so with the product's flags; always
    compiles (the headers under test are not tracked by any timestamp)."""
    so = os.path.join(str(out_dir), f"lib{name}.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-shared",
                    "-std=c++17", "-I", os.path.join(ROOT, "ggrs_amd", "csrc"),
                    os.path.join(HERE, "native", f"{name}.hip"), "-o", so], check=True)
    return so


def f2u(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def u2f(a):
    return np.ascontiguousarray(a, np.uint32).view(F32)


def bits_of(x):
    """the bit pattern of one float32 value, as an int"""
    return int(np.array(x, F32).reshape(1).view(np.uint32)[0])


def _bits(base, deltas):
    """bit patterns base + deltas (base a float or a bit pattern), as uint32"""
    b = bits_of(base) if isinstance(base, (float, np.floating)) else int(base)
    return (b + np.asarray(deltas, np.int64)).astype(np.uint32)


def _states(x, y, vx, vy, rot_bits):
    """[n][5] uint32 from broadcastable float x, y, vx, vy and rotation BITS"""
    x, y, vx, vy = (np.asarray(a, F32) for a in (x, y, vx, vy))
    rot = u2f(np.asarray(rot_bits, np.uint32))
    cols = np.broadcast_arrays(x, y, vx, vy, rot)
    return np.stack([f2u(c.ravel()) for c in cols], axis=1)


def _rand_rot(rng, n):
    """in-domain rotation bits: even lanes uniform over the bit patterns 0 .. kTwoPiBits (every
    exponent, mostly small angles), odd lanes uniform over the angles [0, 2 pi]"""
    r = rng.integers(0, TWO_PI_BITS + 1, n).astype(np.uint32)
    angle = f2u((rng.random(n) * (2.0 * np.pi)).astype(F32))
    r[1::2] = np.minimum(angle, np.uint32(TWO_PI_BITS))[1::2]
    return r


def _uniform(rng, n):
    return _states(rng.random(n) * 600.0, rng.random(n) * 800.0, rng.uniform(-8.0, 8.0, n), rng.uniform(-8.0, 8.0, n),
                   _rand_rot(rng, n))


def _walls(rng):
    out = []
    up, dn = lambda v: np.nextafter(F32(v), F32(np.inf)), lambda v: np.nextafter(F32(v), F32(-np.inf))
    vs = np.array([3.0, -3.0, 0.5, -0.5, 7.5, -7.5], F32)
    for bound, axis in ((600.0, 0), (800.0, 1)):
        edge = np.array([0.0, up(0.0), bound, dn(bound)], F32)
        e, v = (a.ravel() for a in np.meshgrid(edge, vs))
        mid, side = F32(400.0 if axis == 0 else 300.0), F32(0.25)
        out.append(_states(e, mid, v, side, _rand_rot(rng, e.size)) if axis == 0 else
                   _states(mid, e, side, v, _rand_rot(rng, e.size)))
        # x = -(v * 0.98f): the sum with the decayed velocity is +0; and its two neighbours (-1 ulp
        # outside, +1 ulp inside).  x = T - t for T = bound and its neighbours: 1 ulp inside / outside.
        for v0 in (3.0, 0.3, 7.0):
            t_neg, t_pos = F32(-v0) * FRICTION, F32(v0) * FRICTION
            pos = [dn(-t_neg), -t_neg, up(-t_neg)]
            for T in (dn(bound), F32(bound), up(bound)):
                x = F32(T - t_pos)
                for cand in (x, up(x), dn(x)):
                    if F32(cand + t_pos) == T and cand <= F32(bound):
                        pos.append(cand)
                        break
                else:
                    raise AssertionError("no position lands the sum on the wanted neighbour of the bound")
            pos = np.array(pos, F32)
            vel = np.array([-v0] * 3 + [v0] * 3, F32)
            out.append(_states(pos, mid, vel, 0.0, _rand_rot(rng, 6)) if axis == 0 else
                       _states(mid, pos, 0.0, vel, _rand_rot(rng, 6)))
    cx, cy, cvx, cvy = (a.ravel() for a in np.meshgrid([0.0, 600.0], [0.0, 800.0], [3.0, -3.0], [3.0, -3.0]))
    out.append(_states(cx, cy, cvx, cvy, _rand_rot(rng, cx.size)))
    return np.concatenate(out)


def _clamp_threshold(rng):
    out = []
    c = F32(7.0) / FRICTION
    near = _bits(c, np.arange(-64, 65))
    near = np.concatenate([near, near | np.uint32(0x80000000)])
    for other in (0x00000000, 0x80000000, 0x00012345):  # +0, -0, a subnormal
        o = u2f(np.full(near.size, other, np.uint32))
        out.append(_states(300.0, 400.0, u2f(near), o, _rand_rot(rng, near.size)))
        out.append(_states(300.0, 400.0, o, u2f(near), _rand_rot(rng, near.size)))
    th = 2.0 * np.pi * np.arange(4096) / 4096.0
    vx0, vy0 = f2u((float(c) * np.cos(th)).astype(F32)), f2u((float(c) * np.sin(th)).astype(F32))
    for j in range(-3, 4):  # the magnitude of vx moved j ulps
        vx = (vx0.astype(np.int64) + j).astype(np.uint32)
        out.append(_states(rng.random(4096) * 500.0 + 50.0, rng.random(4096) * 700.0 + 50.0, u2f(vx), u2f(vy0),
                           _rand_rot(rng, 4096)))
    return np.concatenate(out)


def _velocity_specials(rng):
    v = u2f(np.array([0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000], np.uint32))
    rots = np.concatenate([_rand_rot(rng, 8), np.array([0, TWO_PI_BITS], np.uint32)])
    pos = np.array([[300.0, 400.0], [0.0, 800.0]], F32)
    vx, vy, r, p = (a.ravel() for a in np.meshgrid(v, v, np.arange(rots.size), np.arange(2)))
    return _states(pos[p, 0], pos[p, 1], vx, vy, rots[r])


def rotation_edges():
    """in-domain rotation bit patterns at the edges of the turn and of the sin/cos reduction"""
    two_pi = u2f(np.array([TWO_PI_BITS], np.uint32))[0]
    around = np.arange(-4, 5)
    parts = [np.array([0, 1], np.uint32), _bits(ROTATION_SPEED, around), _bits(F32(two_pi - ROTATION_SPEED), around),
             _bits(TWO_PI_BITS, np.arange(-4, 1))]
    parts += [_bits(F32(k * np.pi / 4.0), around) for k in range(1, 8)]
    r = np.concatenate(parts)
    assert (r <= TWO_PI_BITS).all()
    return r


def _rotation_edge_states():
    rots = rotation_edges()
    vel = np.array([[0.0, 0.0], [1.5, -2.5], [-6.9, 1.0], [5.0, 5.1], [0.1, -0.0], [-7.2, -3.0]], F32)
    pos = np.array([[300.0, 400.0], [599.9, 0.1]], F32)
    r, v, p = (a.ravel() for a in np.meshgrid(np.arange(rots.size), np.arange(vel.shape[0]), np.arange(2)))
    return _states(pos[p, 0], pos[p, 1], vel[v, 0], vel[v, 1], rots[r])


def out_of_domain_rotations(rng):
    neg_rs, b120 = bits_of(-ROTATION_SPEED), bits_of(120.0)
    parts = [np.array([0x80000000, 0x80000001, neg_rs - 1, neg_rs], np.uint32),          # -0, (-RS, 0), -RS
             rng.integers(0x80000001, neg_rs, 200).astype(np.uint32),
             _bits(TWO_PI_BITS, np.arange(1, 5)), np.array([b120 - 1], np.uint32),        # (2 pi, 120)
             rng.integers(TWO_PI_BITS + 1, b120, 300).astype(np.uint32),
             (rng.integers(neg_rs + 1, b120 | 0x80000000, 100)).astype(np.uint32)]       # (-120, -RS)
    for e in range(133, 254):  # |rot| in [120, 2^127): every exponent, both signs
        lo = 0x700000 if e == 133 else 0
        man = np.concatenate([[lo, 0x7FFFFF], rng.integers(lo, 0x800000, 2)]).astype(np.uint32)
        mag = (np.uint32(e) << np.uint32(23)) | man
        parts += [mag, mag | np.uint32(0x80000000)]
    r = np.concatenate(parts).astype(np.uint32)
    assert (r > TWO_PI_BITS).all() and np.isfinite(u2f(r)).all()
    return r


def _out_of_domain(rng):
    rots = out_of_domain_rotations(rng)
    n = rots.size
    vx, vy = rng.uniform(-8.0, 8.0, n), rng.uniform(-8.0, 8.0, n)
    vx[::7], vy[::11] = 0.0, 0.0
    return _states(rng.random(n) * 600.0, rng.random(n) * 800.0, vx, vy, rots)


def build_cases(seed=0x6767, n_uniform=1 << 15):
    """dict: players [n][5] u32, inputs [n] u8, cls [n] (1..6, CLASS_NAMES): every class state x the
    16 direction inputs, half of the bytes with random high bits (every form must ignore them)."""
    rng = np.random.default_rng(seed)
    per_class = {1: _uniform(rng, n_uniform), 2: _walls(rng), 3: _clamp_threshold(rng), 4: _velocity_specials(rng),
                 5: _rotation_edge_states(), 6: _out_of_domain(rng)}
    states = np.concatenate([per_class[k] for k in sorted(per_class)])
    state_cls = np.concatenate([np.full(per_class[k].shape[0], k, np.uint8) for k in sorted(per_class)])
    m = states.shape[0]
    players = np.repeat(states, 16, axis=0)
    inputs = np.tile(np.arange(16, dtype=np.uint8), m)
    high = (rng.integers(0, 16, 16 * m).astype(np.uint8) << 4) * (rng.random(16 * m) < 0.5)
    inputs = inputs | high.astype(np.uint8)
    f = u2f(players)
    assert np.isfinite(f).all() and (np.abs(f[:, 2:4]) <= 8.0).all()
    assert (players[:, 0] <= bits_of(600.0)).all() and (players[:, 1] <= bits_of(800.0)).all()  # +0 .. bound, no -0
    return dict(players=players, inputs=inputs, cls=np.repeat(state_cls, 16), states=states, state_cls=state_cls)


def annotate(oracle, cases):
    """The oracle's step of every case (ref [n][5]) and what the step did, from the inputs and the
    oracle alone: mag2 (the squared speed the clamp tests, in float32 as the reference forms it),
    clamp, ood (rotation outside [+0, 2 pi])."""
    pl, inp = cases["players"], cases["inputs"]
    ref = oracle.ship_step_batch(pl, inp)
    # MOVEMENT_SPEED * (cos, sin) of each case's rot: the oracle's step from rest with thrust
    rest = pl.copy()
    rest[:, 0:2] = f2u(np.array([300.0, 400.0], F32))
    rest[:, 2:4] = 0
    d = u2f(oracle.ship_step_batch(rest, np.full(inp.size, UP, np.uint8))[:, 2:4])
    vel = u2f(pl[:, 2:4]) * FRICTION
    thrust = ((inp & 3) == UP)[:, None]
    brake = ((inp & 3) == DOWN)[:, None]
    vel = np.where(thrust, vel + d, np.where(brake, vel - d, vel))
    mag2 = vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1]
    assert mag2.dtype == F32
    clamp = np.sqrt(mag2) > F32(7.0)
    assert (clamp == (mag2 > F32(49.0))).all()
    # the model above is the reference's own arithmetic: an unclamped step keeps exactly this velocity
    assert (f2u(vel)[~clamp] == ref[~clamp, 2:4]).all()
    assert np.isfinite(u2f(ref)).all() and (mag2 < F32(256.0)).all()
    return dict(cases, ref=ref, mag2=mag2, clamp=clamp, ood=pl[:, 4] > TWO_PI_BITS)


def coverage(an):
    """counts the issue requires to be nonzero, from inputs and oracle outputs"""
    pl, inp, ref, clamp = an["players"], an["inputs"], an["ref"], an["clamp"]
    fin, fout = u2f(pl), u2f(ref)
    ccw, cw = (inp & 12) == LEFT, (inp & 12) == RIGHT
    return {
        "clamped": int(clamp.sum()), "not clamped": int((~clamp).sum()),
        "mag2 == 49": int((an["mag2"] == F32(49.0)).sum()),
        "mag2 1 ulp above 49": int((an["mag2"] == np.nextafter(F32(49.0), F32(64.0))).sum()),
        "wall x = 0": int((ref[:, 0] == 0).sum()), "wall x = 600": int((fout[:, 0] == 600.0).sum()),
        "wall y = 0": int((ref[:, 1] == 0).sum()), "wall y = 800": int((fout[:, 1] == 800.0).sum()),
        "sum x + vx == +0 off the wall": int(((ref[:, 0] == 0) & (pl[:, 0] != 0) & (fin[:, 0] == -fout[:, 2])).sum()),
        "wrap 0 -> 2pi": int((ccw & ~an["ood"] & (fout[:, 4] > fin[:, 4])).sum()),
        "wrap 2pi -> 0": int((cw & ~an["ood"] & (fout[:, 4] < fin[:, 4])).sum()),
        "turn lands on exactly 2pi -> 0": int((cw & ~an["ood"] & (ref[:, 4] == 0)).sum()),
        "2pi kept without a turn": int((~ccw & ~cw & (pl[:, 4] == TWO_PI_BITS) & (ref[:, 4] == TWO_PI_BITS)).sum()),
        "velocity output -0": int((ref[:, 2:4] == 0x80000000).any(axis=1).sum()),
        "subnormal velocity output": int((((ref[:, 2:4] & 0x7F800000) == 0) & ((ref[:, 2:4] & 0x7FFFFF) != 0)).any(axis=1).sum()),
        "out of domain": int(an["ood"].sum()),
        "high input bits set": int((inp >> 4 != 0).sum()),
    }


def _pad_off_64(order):
    """a lane count that is no multiple of the wave size (one case repeated, none dropped)"""
    return np.concatenate([order, order[:1]]) if order.size % 64 == 0 else order


def order_sorted(an, idx):
    """order (a) of the cases idx: by class, then not clamping / clamping -- whole waves of each kind"""
    key = an["cls"][idx].astype(np.int64) * 2 + an["clamp"][idx]
    return _pad_off_64(idx[np.argsort(key, kind="stable")])


SPECIAL_WAVES = 8  # per kind, in order_interleaved


def order_interleaved(an, idx):
    """order (b) of the cases idx, a fixed interleave.  First, SPECIAL_WAVES waves of each kind, 63
    lanes of in-domain cases that do not clamp plus exactly one lane that differs: one clamping lane at
    lane 0, at lane 63; if idx holds out-of-domain cases, one such lane at lane 0, at lane 63, at lane
    17.  Then every other case, strided."""
    clamp, ood = an["clamp"][idx], an["ood"][idx]
    plain, c, o = idx[~clamp & ~ood], idx[clamp & ~ood], idx[ood]
    K = SPECIAL_WAVES
    kinds = [(c, 0, 0), (c, 63, 1)] + ([(o, 0, 0), (o, 63, 1), (o, 17, 2)] if o.size else [])
    assert plain.size >= 101 * 63 * K * len(kinds) and c.size >= 3 * K and (o.size == 0 or o.size >= 3 * K)
    fill = plain[(np.arange(63 * K * len(kinds)) * 101) % plain.size].reshape(len(kinds), K, 63)
    assert np.unique(fill).size == fill.size
    waves, used = [], [fill.ravel()]
    for k, (pool, lane, j) in enumerate(kinds):
        odd = pool[np.linspace(0, pool.size - 1, 3 * K).astype(np.int64)[j::3]]  # K picks across the classes, distinct per kind
        used.append(odd)
        for w in range(K):
            waves.append(np.concatenate([fill[k, w, :lane], odd[w:w + 1], fill[k, w, lane:]]))
    head = np.concatenate(waves)
    rest = np.setdiff1d(idx, np.concatenate(used))
    stride = 7919
    while np.gcd(stride, rest.size) != 1:
        stride += 2
    rest = rest[(np.arange(rest.size, dtype=np.int64) * stride) % rest.size]
    order = np.concatenate([head, rest])
    assert np.array_equal(np.sort(order), np.sort(idx))
    return _pad_off_64(order)


def wave_census(an, order):
    """per 64-lane wave of an order: how many lanes clamp / are out of domain, and the lane count"""
    n = order.size
    pad = (-n) % 64
    lanes = np.concatenate([np.ones(n, bool), np.zeros(pad, bool)]).reshape(-1, 64)
    cl = np.concatenate([an["clamp"][order], np.zeros(pad, bool)]).reshape(-1, 64)
    od = np.concatenate([an["ood"][order], np.zeros(pad, bool)]).reshape(-1, 64)
    return dict(lanes=lanes.sum(1), clamp=cl.sum(1), ood=od.sum(1), clamp_lane0=cl[:, 0], clamp_lane63=cl[:, 63],
                ood_lane0=od[:, 0], ood_lane63=od[:, 63])


def player_groups(an, idx, N, per_pattern=100):
    """lanes of N independent player steps, [lanes][N] case indices from idx (in-domain): first, for
    each player i, per_pattern lanes where only player i clamps, then lanes where all do and lanes
    where none does; then order (a) of idx cut into groups of N."""
    clamp = an["clamp"][idx]
    c, plain = idx[clamp], idx[~clamp]
    pick = lambda pool, count, salt: pool[(np.arange(count, dtype=np.int64) * 97 + salt * 1009) % pool.size]
    pats = []
    for i in range(N):
        g = pick(plain, per_pattern * N, i).reshape(per_pattern, N)
        g[:, i] = pick(c, per_pattern, i)
        pats.append(g)
    pats.append(pick(c, per_pattern * N, N).reshape(per_pattern, N))
    pats.append(pick(plain, per_pattern * N, N + 1).reshape(per_pattern, N))
    a = order_sorted(an, idx)
    a = np.concatenate([a, a[:(-a.size) % N]]).reshape(-1, N)
    g = np.concatenate(pats + [a])
    return np.concatenate([g, g[:1]]) if g.shape[0] % 64 == 0 else g


# ---------------------------------------------------------------- whole states and bincode
def state_fields(p):
    return 1 + 5 * p


def fld_offset(p, k):
    """byte offset of SoA word k (frame, (x, y)*, (vx, vy)*, rot*) in bincode(State): box_game.h"""
    return 0 if k == 0 else (20 + 4 * (k - 1) if k <= 2 * p else (28 + 4 * (k - 1) if k <= 4 * p else 36 + 4 * (k - 1)))


def words_to_bincode(p, words):
    """[n][1 + 5p] SoA words -> [n][36 + 20p] bincode bytes (i32 frame, u64 num_players, three
    Vecs each with a u64 length)"""
    w = np.ascontiguousarray(words, np.uint32)
    out = np.zeros((w.shape[0], 36 + 20 * p), np.uint8)
    for off in (4, 12, 20 + 8 * p, 28 + 16 * p):
        out[:, off] = p
    for k in range(state_fields(p)):
        o = fld_offset(p, k)
        out[:, o:o + 4] = np.ascontiguousarray(w[:, k]).view(np.uint8).reshape(-1, 4)
    return out


def bincode_to_words(p, rows):
    r = np.ascontiguousarray(rows, np.uint8)
    out = np.zeros((r.shape[0], state_fields(p)), np.uint32)
    for k in range(state_fields(p)):
        o = fld_offset(p, k)
        out[:, k] = np.ascontiguousarray(r[:, o:o + 4]).view(np.uint32)[:, 0]
    return out


def state_lanes(an, idx, P, seed, waves=512, with_disconnects=False):
    """Whole P-player states from the cases idx: player 0 of lane j is case S[j], where S is the head
    of order (b) (the one-odd-lane waves first) followed by whole waves sampled from order (a);
    players 1.. take S rolled (player 1 by whole waves, the others not).  Returns SoA words
    [n][1 + 5P], packed inputs [n] u32, the disconnected mask [n] u32, and for the oracle inputs
    [n][P] u8 and status [n][P] u8."""
    rng = np.random.default_rng(seed)
    b, a = order_interleaved(an, idx), order_sorted(an, idx)
    blocks = np.linspace(0, a.size // 64 - 1, waves).astype(np.int64)  # first to last whole wave, evenly
    S = np.concatenate([b[:64 * waves], a[(blocks[:, None] * 64 + np.arange(64)[None, :]).ravel()], b[64 * waves:64 * waves + 37]])
    n = S.size
    who = [S, np.roll(S, 64 * 131), np.roll(S, 12345), np.roll(S[::-1], 777)][:P]
    words = np.zeros((n, state_fields(P)), np.uint32)
    frames = rng.integers(0, 0x7FFFFFFF, n).astype(np.uint32)  # (0x7fffffff itself would overflow the i32 frame)
    frames[:4] = [0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFE]
    words[:, 0] = frames
    inputs = np.zeros((n, P), np.uint8)
    for i, s in enumerate(who):
        pl = an["players"][s]
        words[:, 1 + 2 * i], words[:, 2 + 2 * i] = pl[:, 0], pl[:, 1]
        words[:, 1 + 2 * P + 2 * i], words[:, 2 + 2 * P + 2 * i] = pl[:, 2], pl[:, 3]
        words[:, 1 + 4 * P + i] = pl[:, 4]
        inputs[:, i] = an["inputs"][s]
    disc = np.zeros(n, np.uint32)
    if with_disconnects:
        disc = (rng.integers(0, 1 << P, n) * (rng.random(n) < 0.25)).astype(np.uint32)
    bit = (disc[:, None] >> np.arange(P)[None, :]) & 1
    status = np.where(bit == 1, 2, rng.integers(0, 2, (n, P))).astype(np.uint8)  # Disconnected, else Confirmed / Predicted
    packed = (inputs.astype(np.uint32) << (8 * np.arange(P, dtype=np.uint32))[None, :]).sum(axis=1).astype(np.uint32)
    return dict(words=words, packed=packed, disc=disc, inputs=inputs, status=status, who=who)


def chain_cases(an, seed, steps=8):
    """one lane per in-domain class state (classes 1..5, class order) and `steps` input bytes each:
    a third of the lanes hold one input throughout (so rotations wrap and speeds reach the clamp),
    the rest draw every byte; high bits random."""
    rng = np.random.default_rng(seed)
    st = an["states"][an["state_cls"] != 6]
    n = st.shape[0]
    inp = rng.integers(0, 256, (n, steps)).astype(np.uint8)
    held = rng.random(n) < 1.0 / 3.0
    inp[held] = (inp[held] & 0xF0) | (inp[held, :1] & 0x0F)
    if n % 64 == 0:
        st, inp = np.concatenate([st, st[:1]]), np.concatenate([inp, inp[:1]])
    return st, inp


def fletcher_words(P, seed, n_random=4096):
    """[n][1 + 5P] words for the Fletcher KAT: random; all ones (the largest doubled sums); all
    zero; bytes 254 / 255 alternating; the frame words 0x80000000 and 0x7fffffff over random
    fields; one random field among all-ones."""
    rng = np.random.default_rng(seed)
    F = state_fields(P)
    rnd = lambda n: rng.integers(0, 1 << 32, (n, F), dtype=np.uint64).astype(np.uint32)
    rows = [rnd(n_random), np.full((1, F), 0xFFFFFFFF, np.uint32), np.zeros((1, F), np.uint32)]
    for a, b in ((0xFEFFFEFF, 0xFEFFFEFF), (0xFFFEFFFE, 0xFFFEFFFE), (0xFEFEFEFE, 0xFFFFFFFF), (0xFFFFFFFF, 0xFEFEFEFE)):
        r = np.zeros((1, F), np.uint32)
        r[0, 0::2], r[0, 1::2] = a, b
        rows.append(r)
    for frame in (0x80000000, 0x7FFFFFFF):
        r = rnd(16)
        r[:, 0] = frame
        rows += [r, np.full((1, F), 0xFFFFFFFF, np.uint32)]
        rows[-1][0, 0] = frame
    one = np.full((F, F), 0xFFFFFFFF, np.uint32)
    one[np.arange(F), np.arange(F)] = rng.integers(0, 1 << 32, F, dtype=np.uint64).astype(np.uint32)
    rows.append(one)
    return np.concatenate(rows)


def prepared(oracle):
    """Everything the KATs share, built once: the annotated cases, the index sets (all classes / the
    in-domain classes 1..5), both lane orders of each, and the coverage and wave-layout asserts --
    all from the inputs and the oracle's outputs."""
    an = annotate(oracle, build_cases())
    cov = coverage(an)
    missing = [k for k, v in cov.items() if v <= 0]
    assert not missing, f"the cases do not cover: {missing}"
    every = np.arange(an["inputs"].size)
    lean = np.flatnonzero(an["cls"] != 6)
    assert not an["ood"][lean].any() and an["ood"][an["cls"] == 6].all()
    orders = {("all", "sorted"): order_sorted(an, every), ("all", "interleaved"): order_interleaved(an, every),
              ("lean", "sorted"): order_sorted(an, lean), ("lean", "interleaved"): order_interleaved(an, lean)}
    layout = {}
    for (which, name), o in orders.items():
        assert o.size % 64 != 0 and np.array_equal(np.unique(o), every if which == "all" else lean)
        w = wave_census(an, o)
        full = w["lanes"] == 64
        if name == "sorted":
            layout[which, "whole waves that clamp"] = int((w["clamp"] == 64).sum())
            layout[which, "whole waves that do not clamp"] = int((full & (w["clamp"] == 0)).sum())
            layout[which, "whole waves in the domain"] = int((full & (w["ood"] == 0)).sum())
            if which == "all":
                layout[which, "whole waves out of the domain"] = int((w["ood"] == 64).sum())
        else:
            layout[which, "waves whose one clamping lane is lane 0"] = int(((w["clamp"] == 1) & w["clamp_lane0"]).sum())
            layout[which, "waves whose one clamping lane is lane 63"] = int(((w["clamp"] == 1) & w["clamp_lane63"]).sum())
            if which == "all":
                layout[which, "waves whose one out-of-domain lane is lane 0"] = int(((w["ood"] == 1) & w["ood_lane0"]).sum())
                layout[which, "waves whose one out-of-domain lane is lane 63"] = int(((w["ood"] == 1) & w["ood_lane63"]).sum())
                layout[which, "waves that mix out-of-domain and in-domain lanes"] = int(((w["ood"] > 0) & (w["ood"] < w["lanes"])).sum())
    missing = [k for k, v in layout.items() if v <= 0]
    assert not missing, f"the lane orders do not hold: {missing}"
    return dict(an=an, every=every, lean=lean, orders=orders, coverage=cov, layout=layout)
