"""Named inputs of the phase-function queries (include/tor_phase.h), about 250 rows each: the tables of tests/media_inputs.py with 1
medium, 2 overlapping, 3 nested, the row of 64, a medium of sigma 0 inside an active set and a moving boundary, each with
asymmetries mixed from {0, -0.0, +-2^-20, 0.3, -0.7, +-0.99}; the collisions are media_restatement.march's own (t and the active
word), the rays that escaped get seeded active words instead, and fixed rows get the word 0, a bit at n_media and every bit.  The
incoming directions include (0, 0, +-1), (x, y, -0.0), one tiny component and the lengths 1e-170, 1e150 and 1e160 (the first and
the last: no answer).  `crafted` holds generator states built by inverting the generator's step (an invertible linear map over
GF(2)), so that the first, second or third output is a chosen word: u = 0 three times (the all-zero state), u_sel at its largest,
u_cos at both ends for g = 0.3, 0.99 and the g the clamp search found (CLAMP_G), u_phi at both ends; `fallback` a medium of subnormal sigma, the only kind of table for which the selection's fallback decides.  Every case is a dict of recs, objects,
sigma, albedo, g, rays (n, 7), t (n,), active (n,) uint64, states (n, 4) uint64 and out (n, 7), the evaluation's directions.
assert_coverage() shows on the restatement alone that each case does what its name says."""
import numpy as np

import media_inputs as MI
import media_restatement as MR
import phase_restatement as R

MASK = (1 << 64) - 1
ALL_ONES = MASK
G_SET = [0.0, -0.0, 2.0 ** -20, -(2.0 ** -20), 0.3, -0.7, 0.99, -0.99]


# ---- the generator (support/rng.nim:58-74, xoshiro256+) and the inverse of its step --------------------------------------------------

def step(s):
    s0, s1, s2, s3 = s
    out = (s0 + s3) & MASK
    t = (s1 << 17) & MASK
    s2 ^= s0
    s3 ^= s1
    s1 ^= s2
    s0 ^= s3
    s2 ^= t
    s3 = ((s3 << 45) | (s3 >> 19)) & MASK
    return out, (s0, s1, s2, s3)


def unstep(s):
    """The state whose step gives `s`: s3' = rotl(s3 ^ s1, 45), s0' = s0 ^ s3 ^ s1, s1' = s1 ^ s2 ^ s0, s2' = s2 ^ s0 ^ (s1 << 17);
    so s1 ^ (s1 << 17) = s1' ^ s2', solved by y ^ (y << 17) ^ (y << 34) ^ (y << 51)."""
    n0, n1, n2, n3 = s
    x = ((n3 >> 45) | (n3 << 19)) & MASK          # s3 ^ s1
    s0 = n0 ^ x
    y = n1 ^ n2
    s1 = (y ^ (y << 17) ^ (y << 34) ^ (y << 51)) & MASK
    s2 = n1 ^ s1 ^ s0
    s3 = x ^ s1
    return (s0, s1, s2, s3)


def state_with(position, word, filler):
    """A state whose output number `position` (0, 1 or 2) is `word`; filler: two words that make the rest of it."""
    s = (word, filler[0], filler[1], 0)           # s0 + s3 == word
    for _ in range(position):
        s = unstep(s)
    return s


def outputs(s, k=3):
    got = []
    for _ in range(k):
        o, s = step(s)
        got.append(o)
    return got


def uniform_of(word):
    return float((word >> 12) * 2.0 ** -52)       # rng.nim:129-133: the top 52 bits


U_MAX = uniform_of(ALL_ONES)                      # 1 - 2^-52: the largest uniform01 there is


def derived_states(states, constant=0x9e3779b97f4a7c15):
    """integrators._derived_states, restated on uint64 words (the light-draw states of trace_direct and trace_media_direct)."""
    st = np.ascontiguousarray(states).view(np.uint64).reshape(-1, 4)
    out = np.empty_like(st)
    mix = 0xbf58476d1ce4e5b9
    for i in range(st.shape[0]):
        w = [int(v) for v in st[i]]
        for k in range(4):
            nxt = w[(k + 1) % 4]
            z = ((w[k] ^ (((nxt << 23) | (nxt >> 41)) & MASK)) + (((k + 1) * constant) & MASK)) & MASK
            z = ((z ^ (z >> 30)) * mix) & MASK
            z = ((z ^ (z >> 27)) * mix) & MASK
            out[i, k] = z ^ (z >> 31)
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1))[..., None]


DIRECTION_ROWS = {}


def _directions(rays):
    """The named incoming directions, written over rows 8 .. of a case's rays."""
    named = [("plus_z", (0.0, 0.0, 1.0)), ("minus_z", (0.0, 0.0, -1.0)), ("minus_z_long", (0.0, 0.0, -2.5)),
             ("negative_zero_z", (0.6, -0.8, -0.0)), ("positive_zero_z", (0.6, -0.8, 0.0)), ("tiny_x", (1e-300, 0.3, -0.4)),
             ("tiny_z", (0.3, 0.4, -1e-300)), ("length_1e-170", tuple(1e-170 * _unit([1.0, 2.0, -2.0]))),
             ("length_1e150", tuple(1e150 * _unit([1.0, 2.0, -2.0]))), ("length_1e160", tuple(1e160 * _unit([1.0, 2.0, -2.0]))),
             ("nan_x", (np.nan, 1.0, 0.0)), ("inf_y", (0.0, np.inf, 1.0)), ("zero", (0.0, 0.0, 0.0)),
             ("near_minus_z", (1e-9, -1e-9, -1.0))]
    for k, (name, d) in enumerate(named):
        DIRECTION_ROWS[name] = 8 + k
        rays[8 + k, 3:6] = d
    return rays


def _case(name, base, gs, seed, reps=4):
    c = MI.BY_NAME[base]
    g = np.random.default_rng(seed)
    M = len(c["objects"])
    rays = np.tile(c["rays"], (reps, 1))[:260] if len(c["rays"]) < 200 else c["rays"].copy()
    tau = np.tile(c["tau"], reps)[:len(rays)] if len(c["rays"]) < 200 else c["tau"].copy()
    tau = np.where(np.isfinite(tau), tau * g.uniform(0.2, 1.0, len(tau)), tau)
    n = len(rays)
    m = MR.march(c["recs"], c["objects"], c["sigma"], rays, tau, None)
    t, active = m["t"].copy(), m["active"].copy()
    escaped = m["status"] != MR.COLLIDED
    t[escaped] = g.uniform(0.0, 2.0, int(escaped.sum()))
    words = g.integers(1, 1 << min(M, 62), size=n, dtype=np.uint64) & g.integers(0, 1 << 62, size=n, dtype=np.uint64) if M > 1 else np.ones(n, dtype=np.uint64)
    if M == 64:
        words |= np.where(g.random(n) < 0.2, np.uint64(1) << np.uint64(63), np.uint64(0))
    words[words == 0] = 1
    active[escaped] = words[escaped]
    rays = _directions(rays.copy())
    active[8:8 + len(DIRECTION_ROWS)] = np.uint64((1 << M) - 1)                      # the named directions: every medium active
    active[0] = 0
    active[1] = np.uint64(1) << np.uint64(M) if M < 64 else np.uint64(0)             # a bit at n_media: no answer
    active[2] = np.uint64((1 << M) - 1)                                              # every medium at once
    active[3] = np.uint64(((1 << M) - 1) | (1 << 63)) if M < 63 else np.uint64(0)    # ... and one far above
    out = np.zeros((n, 7))
    out[:, 3:6] = _unit(g.normal(size=(n, 3))) * g.choice([1.0, 0.25, 7.0, 1e150, 1e-150], size=n)[:, None]
    out[4, 3:6], out[5, 3:6] = rays[4, 3:6], -rays[5, 3:6]                           # mu = +-1: the dot product's clamp
    out[6, 3:6], out[7, 3:6] = 1e160 * _unit([1.0, 1.0, 1.0]), 1e-170 * _unit([1.0, 1.0, 1.0])   # no answer
    out[40:48, 3:6] = rays[40:48, 3:6] * g.uniform(0.5, 2.0, (8, 1))                 # forward, where rounding can pass 1
    out[48:56, 3:6] = -rays[48:56, 3:6] * g.uniform(0.5, 2.0, (8, 1))
    return dict(name=name, recs=c["recs"], objects=c["objects"], sigma=c["sigma"], albedo=c["albedo"],
                g=np.asarray(gs, dtype=np.float64), rays=np.ascontiguousarray(rays), t=t, active=active,
                states=MI.states(n, seed + 1000), out=out)


# the g for which the inversion leaves [-1, 1] at an extreme uniform, the first search_clamp(4096, 3) reports on each side:
# (g, u_cos, the unclamped cosine); set below, after the search
CLAMP_G = None


def search_clamp(n, seed):
    """The (g, u_cos) with u_cos in {0, U_MAX} and TOR_PHASE_G_MIN <= |g| <= TOR_PHASE_G_MAX whose unclamped cosine lies outside
    [-1, 1]: rows (g, u_cos, raw)."""
    gen = np.random.default_rng(seed)
    found = []
    for g in np.concatenate([[0.3, 0.99, -0.99, -0.7, 2.0 ** -20], gen.uniform(-0.99, 0.99, n)]):
        if abs(g) < R.G_MIN:
            continue
        for u in (0.0, U_MAX):
            raw = R.cosine(float(g), u, "no_clamp")[1]
            if raw > 1.0 or raw < -1.0:
                found.append((float(g), u, raw))
    return found


CRAFTED_ROWS = {}


def _crafted():
    """Three overlapping unit-scale media with g = (0.3, 0.99, CLAMP_G's) and a fourth of sigma 0; every row has all four active."""
    recs = [MI._sphere((0, 0, 0), 2.0), MI._sphere((0.1, 0, 0), 2.0), MI._sphere((0, 0.1, 0), 2.0), MI._sphere((0, 0, 0.1), 2.0)]
    sigma = [0.25, 0.5, 0.25, 0.0]
    albedo = [[0.9, 0.5, 0.1], [0.2, 0.8, 0.6], [1.0, 1.0, 1.0], [0.3, 0.3, 0.3]]
    g_lo, g_hi = CLAMP_G[0][0], CLAMP_G[1][0]
    gs = [0.3, 0.99, g_lo, g_hi]
    fill = np.random.default_rng(5).integers(1, 1 << 63, size=(64, 2), dtype=np.uint64)
    rows, act = [], []

    def add(name, state, active=0b1111):
        CRAFTED_ROWS[name] = len(rows)
        rows.append([int(v) for v in state])
        act.append(active)
    CRAFTED_ROWS.clear()
    f = lambda k: (int(fill[k, 0]), int(fill[k, 1]))
    add("all_zero", (0, 0, 0, 0))
    add("all_zero_first_medium", (0, 0, 0, 0), 0b0001)
    add("u_sel_max", state_with(0, ALL_ONES, f(0)))                       # x = U_MAX * rho: the last medium with sigma > 0
    add("u_sel_max_sigma0_last", state_with(0, ALL_ONES, f(1)), 0b1011)
    add("u_sel_zero", state_with(0, 0, f(2)))
    add("u_sel_on_boundary", state_with(0, 1 << 62, f(3)))                # u_sel = 0.25: x == acc after medium 0 (x < acc is strict)
    add("u_sel_on_second_boundary", state_with(0, 3 << 62, f(4)))         # u_sel = 0.75: x == acc after medium 1
    for k, (name, active) in enumerate((("g03", 0b0001), ("g099", 0b0010), ("g_lo", 0b0100))):
        add(f"u_cos_zero_{name}", state_with(1, 0, f(5 + k)), active)
        add(f"u_cos_max_{name}", state_with(1, ALL_ONES, f(8 + k)), active)
    add("u_phi_zero", state_with(2, 0, f(11)))
    add("u_phi_max", state_with(2, ALL_ONES, f(12)))
    add("u_phi_quarter", state_with(2, 1 << 62, f(13)))
    n = len(rows)
    gen = np.random.default_rng(6)
    extra = 200 - n                                                        # seeded rows: every subset of the four, often
    for k in range(extra):
        rows.append([int(v) for v in gen.integers(1, 1 << 63, size=4, dtype=np.uint64)])
        act.append(int(gen.integers(1, 16)))
    n = len(rows)
    rays = np.zeros((n, 7))
    rays[:, 0:3] = gen.normal(size=(n, 3)) * 0.2
    rays[:, 3:6] = _unit(gen.normal(size=(n, 3))) * gen.uniform(0.3, 3.0, n)[:, None]
    rays[:, 6] = gen.random(n)
    rays[CRAFTED_ROWS["u_cos_zero_g099"], 3:6] = (0.0, 0.0, -1.0)          # mu = -1 around -z: v = +z through the copysign frame
    out = np.zeros((n, 7))
    out[:, 3:6] = _unit(gen.normal(size=(n, 3)))
    return dict(name="crafted", recs=np.asarray(recs, dtype=np.float64), objects=np.arange(4, dtype=np.int32),
                sigma=np.asarray(sigma), albedo=np.asarray(albedo), g=np.asarray(gs), rays=rays, t=gen.uniform(0.0, 1.0, n),
                active=np.asarray(act, dtype=np.uint64), states=np.asarray(rows, dtype=np.uint64), out=out)


FALLBACK_ROWS = {}


def _fallback():
    """Two media, the first of a subnormal sigma = 2^-1030, the second of sigma 0.  uniform01 keeps 52 bits, so u_sel <= 1 - 2^-52,
    and for a normal rho the product u_sel * rho rounds to a value below rho: the header's fallback then never decides.  Below
    2^-1023 the spacing of float64 is 2^-1074 > rho * 2^-52 * 2, so (1 - 2^-52) * rho rounds back to rho: x == acc at the last
    medium, `x < acc` never holds, and the fallback picks the last medium with sigma > 0 -- medium 0, not the medium of sigma 0
    behind it.  Rows 0 .. 3 have u_sel at its largest; the rest are seeded."""
    recs = [MI._sphere((0, 0, 0), 2.0), MI._sphere((0.1, 0, 0), 2.0)]
    gen = np.random.default_rng(8)
    rows = [state_with(0, ALL_ONES, (int(a), int(b))) for a, b in gen.integers(1, 1 << 63, size=(4, 2), dtype=np.uint64)]
    act = [0b11, 0b01, 0b11, 0b11]
    FALLBACK_ROWS.update(sigma0_behind=0, alone=1, again=2, minus_z=3)
    n = 200
    rows += [tuple(int(v) for v in gen.integers(1, 1 << 63, size=4, dtype=np.uint64)) for _ in range(n - 4)]
    act += [int(v) for v in gen.integers(1, 4, size=n - 4)]
    rays = np.zeros((n, 7))
    rays[:, 0:3] = gen.normal(size=(n, 3)) * 0.2
    rays[:, 3:6] = _unit(gen.normal(size=(n, 3))) * gen.uniform(0.3, 3.0, n)[:, None]
    rays[3, 3:6] = (0.0, 0.0, -1.0)
    out = np.zeros((n, 7))
    out[:, 3:6] = _unit(gen.normal(size=(n, 3)))
    return dict(name="fallback", recs=np.asarray(recs, dtype=np.float64), objects=np.arange(2, dtype=np.int32),
                sigma=np.asarray([2.0 ** -1030, 0.0]), albedo=np.asarray([[0.9, 0.5, 0.1], [0.2, 0.8, 0.6]]), g=np.asarray([0.3, 0.99]),
                rays=rays, t=gen.uniform(0.0, 1.0, n), active=np.asarray(act, dtype=np.uint64), states=np.asarray(rows, dtype=np.uint64),
                out=out)


def _build():
    cases = [
        _case("one", "one", [0.3], 101),
        _case("one_isotropic", "one", [-0.0], 102),
        _case("two_overlap", "two_overlap", [-0.7, 0.99], 103),
        _case("nested3", "nested3", [2.0 ** -20, 0.3, -0.99], 104),
        _case("row64", "row64", [G_SET[m % 8] for m in range(64)], 105),
        _case("sigma0", "sigma0", [0.99, -(2.0 ** -20)], 106),
        _case("moving", "moving", [0.0, -0.7], 107),
    ]
    if CLAMP_G is not None:
        cases.append(_crafted())
    cases.append(_fallback())
    return cases


CLAMP_G = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))   # replaced below by the search's first finds below -1 and above +1
_found = search_clamp(4096, 3)
_below = [r for r in _found if r[2] < -1.0]
_above = [r for r in _found if r[2] > 1.0]
CLAMP_G = (_below[0], _above[0]) if _below and _above else None
CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]


def lists():
    return MI.lists()           # over row64's 257 rays: 1, 63, 64, 65 and 257 entries (two of the last outside [0, n))


def answer(oracle, c, index=None, into=None, variant=None, details=None):
    return R.sample(oracle, c["sigma"], c["albedo"], c["g"], c["rays"], c["t"], c["active"], c["states"], index, into, variant, details)


def evaluation(c, index=None, into=None, variant=None):
    return R.evaluate(c["sigma"], c["albedo"], c["g"], c["rays"], c["active"], c["out"], index, into, variant)


def physics_case(g, n=4096, seed=41):
    """n draws from one medium of asymmetry g: rays with seeded unit-scale directions, every active word 1."""
    gen = np.random.default_rng(seed)
    rays = np.zeros((n, 7))
    rays[:, 3:6] = _unit(gen.normal(size=(n, 3))) * gen.uniform(0.5, 2.0, n)[:, None]
    return dict(name=f"physics_{g}", recs=MI.PHYSICS_RECS, objects=np.asarray([0], dtype=np.int32), sigma=np.asarray([0.5]),
                albedo=np.asarray([[0.9, 0.6, 0.3]]), g=np.asarray([g]), rays=rays, t=np.zeros(n), active=np.ones(n, dtype=np.uint64),
                states=MI.states(n, seed + 1), out=rays)


def hg_cdf(g, x):
    """P(mu <= x) of Henyey-Greenstein, g != 0: (1 - g^2) / (2 g) * (1 / sqrt(1 + g^2 - 2 g x) - 1 / (1 + g))."""
    return (1.0 - g * g) / (2.0 * g) * (1.0 / np.sqrt(1.0 + g * g - 2.0 * g * x) - 1.0 / (1.0 + g))


def cosines(c, res):
    """dot(unit(in), unit(out)) of every sampled row (numpy; for the statistics only)."""
    return (_unit(c["rays"][:, 3:6]) * res["rays"][:, 3:6]).sum(axis=1)


def assert_coverage(oracle):
    """Each case does what its name says, on the restatement alone; returns the measured counts (the floors are half of what was
    measured when the cases were made)."""
    got = {}
    for c in CASES:
        details = {}
        a = answer(oracle, c, details=details)
        e = evaluation(c)
        sampled = (a["pdf"] > 0)
        M = len(c["sigma"])
        pop = np.array([bin(int(v) & ((1 << M) - 1)).count("1") for v in c["active"]])
        chosen = {d["chosen"] for d in details.values() if "chosen" in d}
        got[c["name"]] = dict(n=len(c["rays"]), sampled=int(sampled.sum()), refused=int((~sampled).sum()), multi=int((pop > 1).sum()),
                              chosen=len(chosen), evaluated=int((e["pdf"] > 0).sum()),
                              clamped=sum(1 for d in details.values() if "raw" in d and abs(d["raw"]) > 1.0),
                              eval_clamped=0)
        assert (a["states"] != c["states"]).any(axis=1)[np.asarray(c["states"]).any(axis=1)].all()      # every row drew
        if c["name"] not in ("crafted", "fallback"):
            assert not sampled[0] and not sampled[1] and not e["pdf"][0] and not e["pdf"][1], c["name"]  # word 0, a bit at n_media
            row = DIRECTION_ROWS
            for name in ("length_1e-170", "length_1e160", "nan_x", "inf_y", "zero"):
                assert not sampled[row[name]] and (a["rays"][row[name]] == 0).all() and e["pdf"][row[name]] == 0, (c["name"], name)
            for name in ("plus_z", "minus_z", "minus_z_long", "negative_zero_z", "positive_zero_z", "tiny_x", "tiny_z", "length_1e150",
                         "near_minus_z"):
                assert sampled[row[name]] and np.isfinite(a["rays"][row[name]]).all(), (c["name"], name)
                v = a["rays"][row[name], 3:6]
                assert abs(float((v * v).sum()) - 1.0) <= 1e-14, (c["name"], name)
            assert sampled[2] and pop[2] == M and e["pdf"][2] > 0                                       # every bit
            assert e["pdf"][6] == 0 and e["pdf"][7] == 0                                                # out of 1e160, 1e-170
    for name, (smp, multi) in FLOORS.items():
        assert got[name]["n"] >= 200 and got[name]["sampled"] >= smp and got[name]["multi"] >= multi, (name, got[name])
    assert got["row64"]["chosen"] >= 20 and got["nested3"]["chosen"] == 3 and got["two_overlap"]["chosen"] == 2
    # sigma 0 inside an active set: never chosen, though active
    c = BY_NAME["sigma0"]
    details = {}
    answer(oracle, c, details=details)
    both = [i for i, d in details.items() if "chosen" in d and int(c["active"][i]) & 3 == 3]
    assert len(both) >= 20 and all(details[i]["chosen"] == 1 for i in both)
    # the moving boundary: the collisions of the march depend on the rays' times
    c = BY_NAME["moving"]
    other = c["rays"].copy()
    other[:, 6] = 1.0 - other[:, 6]
    base = MI.BY_NAME["moving"]
    assert (MR.roots(base["recs"], [0], other)[1] != MR.roots(base["recs"], [0], c["rays"])[1]).sum() >= 20
    # the crafted states put the chosen words where they say
    if CLAMP_G is not None:
        c = BY_NAME["crafted"]
        row = CRAFTED_ROWS
        u = lambda name: [uniform_of(o) for o in outputs(tuple(int(v) for v in c["states"][row[name]]))]
        assert u("all_zero") == [0.0, 0.0, 0.0] and u("u_sel_max")[0] == U_MAX == 1.0 - 2.0 ** -52 and u("u_sel_zero")[0] == 0.0
        assert u("u_sel_on_boundary")[0] == 0.25 and u("u_sel_on_second_boundary")[0] == 0.75
        assert u("u_cos_zero_g03")[1] == 0.0 and u("u_cos_max_g099")[1] == U_MAX and u("u_phi_zero")[2] == 0.0 and u("u_phi_max")[2] == U_MAX
        details = {}
        a = answer(oracle, c, details=details)
        d = lambda name: details[row[name]]
        assert d("all_zero")["chosen"] == 0 and d("all_zero")["mu"] == -1.0                      # u = 0: mu = -1 for any g != 0
        assert d("u_sel_max")["chosen"] == 2 and not d("u_sel_max")["fell"]                      # sigma 0 is last: never chosen
        assert d("u_sel_max_sigma0_last")["chosen"] == 1
        assert d("u_sel_on_boundary")["chosen"] == 1 and d("u_sel_on_second_boundary")["chosen"] == 2     # x == acc: strict <
        assert d("u_cos_zero_g_lo")["raw"] < -1.0 and d("u_cos_zero_g_lo")["mu"] == -1.0         # the clamp decides
        v = a["rays"][row["u_cos_zero_g099"], 3:6]
        assert d("u_cos_zero_g099")["mu"] == -1.0 and abs(v[2] - 1.0) <= 1e-15                   # backwards from -z: +z
        assert got["crafted"]["clamped"] >= 1
    # the fallback decides, and picks the medium in front of the one of sigma 0
    c = BY_NAME["fallback"]
    details = {}
    a = answer(oracle, c, details=details)
    assert U_MAX * 2.0 ** -1030 == 2.0 ** -1030 and U_MAX * 2.0 ** -1022 < 2.0 ** -1022
    for name, i in FALLBACK_ROWS.items():
        assert details[i]["fell"] and details[i]["chosen"] == 0 and a["pdf"][i] > 0, name
    assert sum(1 for d in details.values() if d.get("fell")) == 4
    return got


# name: (sampled at least, rows with more than one active medium at least): half of what was measured (one 252 / 0, one_isotropic
# 252 / 0, two_overlap 244 / 55, nested3 248 / 168, row64 249 / 252, sigma0 138 / 105, moving 252 / 52, crafted 189 / 154,
# fallback 133 / 70)
FLOORS = {"one": (126, 0), "one_isotropic": (126, 0), "two_overlap": (122, 27), "nested3": (124, 84), "row64": (124, 126),
          "sigma0": (69, 52), "moving": (126, 26), "crafted": (94, 77), "fallback": (66, 30)}
