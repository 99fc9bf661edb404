"""Record normal_sampler.npz: crafted PCG64 states that put the rare branches of NumPy's Generator.standard_normal (256-layer ziggurat) at a chosen
velocity index of a MuJoCo reset, with what NumPy makes of them.  NumPy only: nothing of the project is imported.

    python tests/golden/make_golden_normal_sampler.py          # rewrites tests/golden/normal_sampler.npz

One fixed PCG64 supplies WORDS = 2^24 raw words.  A draw that starts at word j is replayed by `Generator.standard_normal()` on the state `advance(j)`
and classified by the number of raw words it consumed and by |x| > R:

    plain          1 word                                         (the fast path)
    wedge-accept   2 words, |x| < R                               (one exp comparison, accepted)
    wedge-reject   first word idx != 0, here exactly 3 words      (one exp comparison, rejected, then a plain draw)
    tail           3 words, |x| > R                               (idx == 0: two log1p, accepted at once)
    tail-retry     >= 5 words, |x| > R, first word idx == 0       (the tail's rejection loop ran more than once)

All 65 536 words with idx == 0 are replayed (the tail pools), and the first SCAN words one by one (the wedge and plain pools).  For each robot -- HalfCheetah
(nq 9, nv 9), Ant (15, 14), InvertedDoublePendulum (3, 3) -- N = 1024 lanes are built: lane i has its special draw at velocity index k = i % nv, its
state is `advance(j - nq - k)`, so that the nq uniform position draws and k plain normals (verified by replay) come first; the categories (512 tail,
128 tail-retry, 128 wedge-accept, 128 wedge-reject, 128 plain) are dealt evenly to the wavefronts and shuffled inside each, so every wavefront mixes them.

Stored per robot <r>: <r>_words [N, 4] ({state_hi, state_lo, inc_hi, inc_lo}, the layout of gymnasium_amd._native.pcg_words), <r>_category, <r>_k,
<r>_qpos = qpos0 + g.uniform(-0.1, 0.1, nq), <r>_qvel = 0.1 * g.standard_normal(nv), <r>_words_after.  Stored once: the arguments -u and the results, as bit patterns,
of every log1p call of the tail lanes (log1p_x, log1p_r; math.log1p) and of every exp call of the wedge lanes (exp_x, exp_r; math.exp) -- the libm of
the machine the reference runs on (glibc 2.35).  The script replays those calls itself: the tail loop's accept / reject decisions and the value +-(R + (-1/R) log1p(-u)),
recomputed with math.log1p, must be NumPy's; the wedge's x = rabs * wi[idx], with wi recovered from NumPy's own draws, must be the accepted draw.
"""
import io
import math
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "normal_sampler.npz")
SEED = 20240607
WORDS = 1 << 24
SCAN = 60_000
N = 1024
SCALE = 0.1
R = 3.6541528853610087963519472518
INV_R = 0.27366123732975827203338247596
CATEGORIES = ("plain", "wedge_accept", "wedge_reject", "tail", "tail_retry")
MIX = {"tail": 512, "tail_retry": 128, "wedge_accept": 128, "wedge_reject": 128, "plain": 128}
ROBOTS = {  # name -> (nq, nv, qpos0): the compiled models' (tests/test_normal_sampler.py compares)
    "half_cheetah": (9, 9, np.zeros(9)),
    "ant": (15, 14, np.array([0.0, 0.0, 0.75, 1.0] + [0.0] * 11)),
    "inverted_double_pendulum": (3, 3, np.zeros(3)),
}
CENSUS = {"tail": 4015, "tail_retry": 275}  # of the 65 536 idx == 0 words of this stream (4 290 tail draws in 2^24 words: one in ~3 900)
MAX_K = max(nv for _, nv, _ in ROBOTS.values()) - 1
_M64 = (1 << 64) - 1


def expected_libm():
    """glibc 2.35's log1p and exp, at arguments where its result is NOT the correctly rounded one (which ends in ...77, ...eb, ...d3): a libm that is
    merely accurate fails this"""
    got = (math.log1p(float.fromhex("-0x1.060d7be6f245cp-1")).hex(), math.log1p(float.fromhex("-0x1.3f50be80ff35cp-2")).hex(), math.exp(float.fromhex("-0x1.827e8dc83834ap+2")).hex())
    return got == ("-0x1.6f2460c193076p-1", "-0x1.7eb0d88bd68eap-2", "0x1.3879de9ea4dd4p-9")


class Stream:
    """The fixed generator, its raw words, and replays from any word index."""

    def __init__(self):
        self.bg = np.random.PCG64(SEED)
        self.base = self.bg.state
        self.raw = self.bg.random_raw(WORDS + 64)
        self.gen = np.random.Generator(self.bg)
        self._cache = {}

    def at(self, j):
        self.bg.state = self.base
        self.bg.advance(j)
        return self.gen

    def words(self, j):
        st = self.at(j).bit_generator.state["state"]
        s, i = st["state"], st["inc"]
        return [s >> 64, s & _M64, i >> 64, i & _M64]

    def consumed_since(self, j):
        """how many raw words the generator, started at word j, has consumed (read off the next word; leaves the generator one word further)"""
        nxt = int(self.bg.random_raw())
        for n in range(0, 400):
            if int(self.raw[j + n]) == nxt:
                return n
        raise AssertionError(j)

    def draw(self, j):
        """(x, words consumed) of the standard normal that starts at word j"""
        if j not in self._cache:
            x = float(self.at(j).standard_normal())
            self._cache[j] = (x, self.consumed_since(j))
        return self._cache[j]

    def draw_chain(self, j, count):
        """words consumed by each of `count` consecutive draws from word j"""
        out = []
        for _ in range(count):
            n = self.draw(j)[1]
            out.append(n)
            j += n
        return out

    def plain_run(self, j):
        """how many draws directly before word j are plain ones, up to MAX_K"""
        run = 0
        while run < MAX_K and j - run - 1 >= 0 and self.draw(j - run - 1)[1] == 1:
            run += 1
        return run

    def double(self, j):
        return float(int(self.raw[j]) >> 11) * (1.0 / 9007199254740992.0)

    def fields(self, j):
        r = int(self.raw[j])
        return r & 0xFF, (r >> 8) & 1, (r >> 9) & 0x000FFFFFFFFFFFFF  # idx, sign, rabs


def classify(s, j):
    idx = s.fields(j)[0]
    x, n = s.draw(j)
    if n == 1:
        return "plain"
    if n == 2 and abs(x) < R:
        return "wedge_accept"
    if idx != 0 and n == 3 and s.draw(j + 2) == (x, 1):
        return "wedge_reject"
    if idx == 0 and n == 3 and abs(x) > R:
        return "tail"
    if idx == 0 and n >= 5 and abs(x) > R:
        return "tail_retry"
    return None  # (a rejected wedge followed by anything but a plain draw: not used)


def pools(s):
    out = {c: [] for c in CATEGORIES}
    census = {c: 0 for c in ("tail", "tail_retry")}
    for j in np.flatnonzero((s.raw[:WORDS] & np.uint64(0xFF)) == 0).tolist():
        c = classify(s, j)
        if c in census:
            census[c] += 1
            if j >= 64:
                out[c].append(j)
    for j in range(64, SCAN):
        c = classify(s, j)
        if c in ("plain", "wedge_accept", "wedge_reject"):
            out[c].append(j)
    return out, census


def layer_widths(s, layers):
    """wi[idx] of the layers named, recovered from the plain draws and the accepted wedge draws of the scan (x = rabs * wi[idx] there; layer 1 has
    no plain draws): the one double near x / rabs that reproduces every such draw of the layer"""
    samples = {i: [] for i in layers}
    for j in range(64, SCAN):
        idx, _, rabs = s.fields(j)
        if idx in samples and s.draw(j)[1] <= 2:
            samples[idx].append((rabs, abs(s.draw(j)[0])))
    out = {}
    for i, rows in samples.items():
        ra, xs = np.array([a for a, _ in rows], dtype=np.float64), np.array([b for _, b in rows])
        assert ra.size >= 20, (i, ra.size)
        w0 = float(xs[np.argmax(ra)] / ra.max())
        found = []
        for step in range(-16, 17):
            w = w0
            for _ in range(abs(step)):
                w = math.nextafter(w, math.inf if step > 0 else -math.inf)
            if np.array_equal(ra * w, xs):
                found.append(w)
        assert len(found) == 1, (i, found)
        out[i] = found[0]
    return out


def tail_calls(s, j):
    """the log1p arguments of the tail draw at word j, in call order, and the value they give"""
    x, n = s.draw(j)
    args = [-s.double(j + 1 + t) for t in range(n - 1)]
    for t in range(0, n - 1, 2):
        xx = -INV_R * math.log1p(args[t])
        yy = -math.log1p(args[t + 1])
        accepted = yy + yy > xx * xx
        assert accepted == (t == n - 3), j
    rabs = s.fields(j)[2]
    assert x == (-(R + xx) if (rabs >> 8) & 1 else R + xx), j
    return args


def wedge_call(s, j, wi):
    """the exp argument of the wedge draw at word j: -x^2 / 2 with x = rabs * wi[idx], which for an accepted draw must be the value NumPy returned (the
    comparison's other side needs fi, which is not recovered here: the outcome is read off the number of words NumPy consumed)"""
    idx, sign, rabs = s.fields(j)
    x = float(rabs) * wi[idx]
    got, n = s.draw(j)
    if n == 2:
        assert got == (-x if sign else x), j
    return -0.5 * x * x


def build_robot(s, name, pool, rng):
    nq, nv, qpos0 = ROBOTS[name]
    wave = np.concatenate([np.full(MIX[c] * 64 // N, CATEGORIES.index(c), dtype=np.uint8) for c in CATEGORIES])  # each wavefront: the mix in small, shuffled
    cats = np.concatenate([rng.permutation(wave) for _ in range(N // 64)])
    order = {c: [pool[c][t] for t in rng.permutation(len(pool[c])).tolist()] for c in CATEGORIES}
    used, starts = {c: set() for c in CATEGORIES}, set()
    cols = {k: [] for k in ("words", "k", "qpos", "qvel", "words_after", "special")}
    for i in range(N):
        c, k = CATEGORIES[cats[i]], i % nv
        j = next(j for j in order[c] if j not in used[c] and j >= nq + k + 1 and j - nq - k not in starts and s.plain_run(j) >= k)
        used[c].add(j)
        start = j - nq - k
        starts.add(start)  # (no two lanes with the same state)
        g = s.at(start)
        qpos = qpos0 + g.uniform(low=-SCALE, high=SCALE, size=nq)
        qvel = SCALE * g.standard_normal(nv)
        st = g.bit_generator.state["state"]
        after = [st["state"] >> 64, st["state"] & _M64, st["inc"] >> 64, st["inc"] & _M64]
        consumed = s.consumed_since(start)
        assert qvel[k] == SCALE * s.draw(j)[0] and all(qvel[m] == SCALE * s.draw(start + nq + m)[0] and s.draw(start + nq + m)[1] == 1 for m in range(k)), (name, i)
        assert consumed == nq + k + s.draw(j)[1] + sum(s.draw_chain(j + s.draw(j)[1], nv - k - 1)), (name, i)
        for key, v in (("words", s.words(start)), ("k", k), ("qpos", qpos), ("qvel", qvel), ("words_after", after), ("special", j)):
            cols[key].append(v)
    out = {"category": cats, "k": np.array(cols["k"], dtype=np.uint8), "qpos": np.array(cols["qpos"]), "qvel": np.array(cols["qvel"]),
           "special": np.array(cols["special"], dtype=np.uint32)}
    for key in ("words", "words_after"):
        out[key] = np.array(cols[key], dtype=np.uint64)
    return out


def generate():
    """name -> array, as stored"""
    s = Stream()
    pool, census = pools(s)
    assert census == CENSUS, census
    rng = np.random.default_rng(SEED + 1)
    arrays, log_args, exp_args = {}, set(), set()
    robots = {name: build_robot(s, name, pool, rng) for name in ROBOTS}
    wedge = sorted({int(j) for r in robots.values() for j, c in zip(r["special"], r["category"]) if CATEGORIES[c] in ("wedge_accept", "wedge_reject")})
    wi = layer_widths(s, {s.fields(j)[0] for j in wedge})
    for name, r in robots.items():
        counts = {c: int((r["category"] == t).sum()) for t, c in enumerate(CATEGORIES)}
        assert counts == MIX, (name, counts)
        for j, c in zip(r["special"].tolist(), r["category"].tolist()):
            if CATEGORIES[c] in ("tail", "tail_retry"):
                log_args.update(tail_calls(s, j))
            elif CATEGORIES[c] in ("wedge_accept", "wedge_reject"):
                exp_args.add(wedge_call(s, j, wi))
        for key, v in r.items():
            if key != "special":
                arrays[f"{name}_{key}"] = v
    lx, ex = np.array(sorted(log_args)), np.array(sorted(exp_args))
    u = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    arrays.update(log1p_x=u(lx), log1p_r=u(np.array([math.log1p(v) for v in lx.tolist()])), exp_x=u(ex), exp_r=u(np.array([math.exp(v) for v in ex.tolist()])))
    return arrays


def npz_bytes(arrays):
    """an .npz with nothing of the day it was written in it: the same arrays give the same bytes"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as zf:
        for name in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            zf.writestr(info, b.getvalue(), compresslevel=9)
    return buf.getvalue()


def load(path=PATH):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    if not expected_libm():
        raise SystemExit("this machine's libm is not the reference's (glibc 2.35): not recording")
    data = npz_bytes(generate())
    with open(PATH, "wb") as f:
        f.write(data)
    print(PATH, len(data), "bytes")
