"""GPU: ONE engine across calls whose geometry changes -- above all fea_context, an argument of every *_frames entry and
of the decoders.  An engine keeps two alternating raw buffer sets (feat, targ, first and, on a noise-aware engine, nat
and nat_row) and grows them only when a capacity is exceeded.  A stream row is layersizes[0] / fea_context floats wide
(/ (fea_context + 1) on a NAT engine), so a capacity counted in ROWS says nothing about the floats a set holds: a call
with a smaller context and no more rows than the set was grown for writes past the allocation.  The sets count feat
and nat in floats (one place: raw_set_acquire in csrc/engine.hip, by the rule of csrc/devbuf_rule.h); these tests hold
them to it.

The principle throughout: a long-lived engine goes through a sequence of calls, and after every call its result equals,
in every bit, that of a fresh engine given only that call (same weights): outputs, CV sums, weights, biases and
scalefactor().  Training engines run without momentum, so that weights, biases and the scale are the whole state a fresh
engine has to be given.  The first forward of a sequence is also held to float64 (bounds64.expect_forward_chain), the
decoded waves to the float64 chain of tests/spec64.py.

The precondition (pure Python, checked when this file is imported and by a test that needs no device): every sequence
below would have overrun a set whose capacity is counted in rows.  It is what keeps these tests from passing for the
wrong reason.

The last section counts device allocations (BPGpu.buffer_stats, mlggd_debug_buffers): "grows only when a capacity is
exceeded" is observed, with the outputs still those of a fresh engine."""
import numpy as np
import pytest

import bounds64 as b6
import nat_model
import spec64

gpu = pytest.mark.gpu
B, NFR, K0, D = 32, 300, 48, 12
LS = [K0, 64, 64, D]
HP = (0.01, 0.0, 1e-5)                                   # no momentum: see above
T = 6                                                    # nat_frames of the NAT engines
PLAIN_CTX = [6, 6, 1, 1, 2, 3, 4, 6, 1]                  # each context twice: BOTH sets are small before the wide call
NAT_CTX = [5, 5, 1, 1, 2, 3, 5]                          # stream rows of 8, 8, 24, 24, 16, 12, 8 floats
NAT_FRAMES = [40, 9, 1, 30, 5, 6, 7, 62, 3, 85, 52]      # 11 utterances, 300 frames
assert sum(NAT_FRAMES) == NFR and len(NAT_FRAMES) == 11

# decoding at 8 kHz: 129 bins, context 7; the narrow stream before it has context 43 (21 floats a row, 60 frames)
FS, DD, DCTX, NARROW_CTX, NARROW_FR, DCAP = 8, 129, 7, 43, 60, 64
DEC_LS = [DCTX * DD, 64, DD]
DEC_NAT_LS = [(DCTX + 1) * DD, 64, DD]
DEC_FRAMES = [40, 38, 43]                                # the batch; its first utterance is also decoded alone
DEC_NAT_CTX = [1, 3]                                     # load_frames_nat before (and after) decoding: rows of 516, 258


# ---------------------------------------------------------------------------------------------------------------------
# the precondition: (rows, ctx, fdim, n_nat) of every acquisition of a raw set, in call order
def stream_width(k0, ctx, nat):
    w, rem = divmod(k0, ctx + (1 if nat else 0))
    assert rem == 0
    return w


def frames_calls(ctxs, nat, rows=NFR, k0=K0, n_nat=0):
    return [(rows, c, stream_width(k0, c, nat), n_nat) for c in ctxs]


def decode_calls(frames, ctx, cap, fdim):
    """the chunks of enhance_waves over the packed frames: n frames and ctx - 1 edge rows per utterance touched"""
    fo = np.concatenate([[0], np.cumsum(frames)])
    out = []
    for a in range(0, int(fo[-1]), cap):
        n = min(cap, int(fo[-1]) - a)
        touched = [u for u in range(len(frames)) if fo[u] < a + n and fo[u + 1] > a]
        out.append((n + len(touched) * (ctx - 1), ctx, fdim, 0))
    return out


def rows_only_overruns(calls):
    """what an engine whose sets count feat and nat in rows would have done: the calls (by index) that write more floats
    than the set they land on holds.  The sets alternate; a set regrows only when rows + ctx + 8 (n_nat + 8) exceeds
    its row capacity, to that many rows of the call's own width."""
    sets = [dict(rows=0, floats=0, nrows=0, nfloats=0) for _ in range(2)]
    bad = []
    for i, (rows, ctx, fdim, n_nat) in enumerate(calls):
        s = sets[i % 2]
        if rows + ctx + 8 > s["rows"]:
            s["rows"], s["floats"] = rows + ctx + 8, (rows + ctx + 8) * fdim
        if n_nat and n_nat + 8 > s["nrows"]:
            s["nrows"], s["nfloats"] = n_nat + 8, (n_nat + 8) * fdim
        if rows * fdim > s["floats"] or (n_nat and n_nat * fdim > s["nfloats"]):
            bad.append(i)
    return bad


def check_growing_pairs(calls):
    """every adjacent pair whose rows get wider: no regrowth by rows, more floats than the old allocation held; the same
    for the noise table.  Returns how many such pairs there are."""
    pairs = 0
    for (r1, c1, f1, m1), (r2, c2, f2, m2) in zip(calls, calls[1:]):
        if f2 <= f1:
            continue
        pairs += 1
        assert r2 + c2 + 8 <= r1 + c1 + 8, (r1, c1, r2, c2)
        assert r2 * f2 > (r1 + c1 + 8) * f1, (r1, c1, f1, r2, f2)
        if m1 and m2:
            assert m2 + 8 <= m1 + 8 and m2 * f2 > (m1 + 8) * f1, (m1, f1, m2, f2)
    return pairs


def dec_first_rows():
    return DEC_FRAMES[0] + DCTX - 1


SEQUENCES = {
    "plain": frames_calls(PLAIN_CTX, False),
    "nat": frames_calls(NAT_CTX, True, n_nat=len(NAT_FRAMES)),
    "decode": (frames_calls([NARROW_CTX] * 2, False, NARROW_FR, DEC_LS[0]) + [(dec_first_rows(), DCTX, DD, 0)] +
               decode_calls(DEC_FRAMES, DCTX, DCAP, DD) + frames_calls([NARROW_CTX], False, NARROW_FR, DEC_LS[0])),
    "decode_nat": (frames_calls(DEC_NAT_CTX, True, NARROW_FR, DEC_NAT_LS[0], n_nat=3) + [(dec_first_rows(), DCTX, DD, 0)] +
                   decode_calls(DEC_FRAMES, DCTX, DCAP, DD) + frames_calls(DEC_NAT_CTX, True, NARROW_FR, DEC_NAT_LS[0], n_nat=3)),
}


def check_precondition():
    for name, calls in SEQUENCES.items():
        assert check_growing_pairs(calls) >= 1, name
        assert rows_only_overruns(calls), name
    # the worked example: context 6 allocates (300 + 6 + 8) x 8 = 2512 floats, context 1 then copies 300 x 48 = 14400
    assert rows_only_overruns(SEQUENCES["plain"])[0] == 2 and (NFR + 6 + 8) * 8 == 2512 and NFR * K0 == 14400
    assert rows_only_overruns(SEQUENCES["nat"])[0] == 2 and (11 + 8) * 8 == 152 and 11 * 24 == 264
    # the decoders' first chunk is the first to overrun after the narrow stream, the narrow NAT streams after decoding
    assert rows_only_overruns(SEQUENCES["decode"])[0] == 2
    assert len(decode_calls(DEC_FRAMES, DCTX, DCAP, DD)) == 2              # the capacity splits the batch
    assert set(rows_only_overruns(SEQUENCES["decode_nat"])) >= {5, 6}
    # the simulation itself: a set counted in floats (the fix) never overruns, and equal contexts never did
    assert not rows_only_overruns(frames_calls([6] * 4, False))


check_precondition()


def test_every_sequence_would_overrun_a_set_counted_in_rows():
    check_precondition()


# ---------------------------------------------------------------------------------------------------------------------
# data and engines
class Chunk:
    """a frame stream of `nfr` frames for context `ctx`, a shuffled sample table with a ragged tail, its expanded rows"""

    def __init__(self, ctx, seed, nat=False, nfr=NFR, frames=None):
        rng = np.random.default_rng(1000 * ctx + seed)
        self.ctx, self.nat_engine = ctx, nat
        fdim = self.fdim = stream_width(K0, ctx, nat)
        self.feat = rng.standard_normal((nfr, fdim)).astype(np.float32)
        self.targ = rng.standard_normal((nfr, D)).astype(np.float32)
        frames = frames or [nfr]
        fo = self.fo = np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)
        assert fo[-1] == nfr
        table = np.array([f for u in range(len(frames)) for f in range(fo[u], fo[u + 1] - ctx + 1)], np.int32)
        self.first = table[rng.permutation(table.size)]
        self.n = self.first.size
        assert self.n % B != 0 and self.n > B
        self.toff = ctx // 2
        self.trows = self.targ[self.first + self.toff]
        if nat:
            self.nat = nat_model.noise_rows(self.feat, fo, T)
            self.nat_row = nat_model.utt_of_frames(fo, self.first)
            self.rows = nat_model.expand(self.feat, self.first, ctx, self.nat, self.nat_row)
        else:
            self.rows = np.ascontiguousarray(self.feat[self.first[:, None] + np.arange(ctx)[None, :]].reshape(self.n, K0))
        assert self.rows.shape == (self.n, K0)

    # the entries under test, plain or _nat
    def tail(self):
        return (self.nat, self.nat_row) if self.nat_engine else ()

    def forward(self, eng):
        f = eng.forward_frames_nat if self.nat_engine else eng.forward_frames
        return f(self.feat, self.first, self.ctx, *self.tail())

    def cv(self, eng):
        f = eng.cv_all_frames_nat if self.nat_engine else eng.cv_all_frames
        return np.array(f(self.feat, self.targ, self.first, self.ctx, self.toff, *self.tail()), np.float32)

    def train(self, eng, **kw):
        f = eng.train_frames_nat if self.nat_engine else eng.train_frames
        return f(self.feat, self.targ, self.first, self.ctx, self.toff, *self.tail(), **kw)

    def load(self, eng):
        f = eng.load_frames_nat if self.nat_engine else eng.load_frames
        f(self.feat, self.targ, self.first, self.ctx, self.toff, *self.tail())


def chunks(kind):
    nat = kind == "nat"
    return [Chunk(c, i, nat, frames=NAT_FRAMES if nat else None) for i, c in enumerate(NAT_CTX if nat else PLAIN_CTX)]


NET = b6.make_net(LS, 5)


def engine(pkg, kind, W=None, b=None, alpha=None, ls=LS, cap=0):
    W, b = (NET if W is None else (W, b))
    eng = pkg.BPGpu(1, 0, ls, B, *HP, W, b, 1.2, 1, max_cache_frames=cap, nat_frames=T if kind.endswith("nat") else 0)
    if alpha is not None:
        eng.set_scalefactor(alpha)
    return eng


def state(eng):
    ws, bs = eng.returnWeights()
    return ws + bs + [eng.scalefactor()]


def same_bits(got, want, what=""):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), "%s tensor %d" % (what, i)


def fresh_from(pkg, kind, st):
    """a fresh engine in the state `st` (weights, biases, scalefactor)"""
    nl = len(LS) - 1
    return engine(pkg, kind, st[:nl], st[nl:2 * nl], st[-1])


ALPHA = np.full(D, 0.7, np.float32)                      # a scale per bin: the log-likelihood of a CV call is finite
_REF = {}


def train_chain(pkg, kind):
    """the states a chain of FRESH engines reaches, one engine per call of the sequence, each begun in the state the one
    before it left (computed once, shared by the training legs)"""
    if kind not in _REF:
        st, out = NET[0] + NET[1] + [ALPHA], []
        for ch in chunks(kind):
            eng = fresh_from(pkg, kind, st)
            assert ch.train(eng) == ch.n // B >= 1
            st = state(eng)
            eng.close()
            assert all(np.isfinite(a).all() for a in st)
            out.append(st)
        assert any(a.tobytes() != b.tobytes() for a, b in zip(out[0], out[-1]))
        _REF[kind] = out
    return _REF[kind]


# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["plain", "nat"])
def test_forward_and_cv_through_the_contexts(pkg, kind):
    """forward_frames, then cv_all_frames with the sums formed on the host and on the device, each through the whole
    sequence on one engine; the first forward also against float64"""
    seq = chunks(kind)
    long = engine(pkg, kind, alpha=ALPHA)
    for i, ch in enumerate(seq):
        got = ch.forward(long)
        ref = engine(pkg, kind, alpha=ALPHA)
        want = ch.forward(ref)
        assert ref.forward(ch.rows).tobytes() == want.tobytes()               # ... which is the expanded rows' output
        ref.close()
        assert got.shape == (ch.n, D) and np.isfinite(got).all() and got.tobytes() == want.tobytes(), (i, ch.ctx)
        if i == 0:
            rep = b6.compare("forward ctx %d" % ch.ctx, got, b6.expect_forward_chain(ch.rows, *NET, long.out_slabs()))
            print(rep.line())
            assert rep.ok, rep.line()
    for on in (False, True):
        long.set_cv_device_reduce(on)
        for i, ch in enumerate(seq):
            got = ch.cv(long)
            ref = engine(pkg, kind, alpha=ALPHA)
            ref.set_cv_device_reduce(on)
            want = ch.cv(ref)
            ref.close()
            assert np.isfinite(got).all() and got.tobytes() == want.tobytes(), (on, i, ch.ctx, got, want)
    long.close()


@gpu
@pytest.mark.parametrize("kind,leg", [("plain", "train_frames"), ("plain", "load_then_resident"), ("plain", "async"),
                                      ("nat", "train_frames"), ("nat", "load_then_resident")])
def test_training_through_the_contexts(pkg, kind, leg):
    """after every call the long-lived engine stands where the chain of fresh engines stands; `async`: the chunks go
    back to back with wait=False and the engine is looked at once, at the end (there is no asynchronous _nat entry)"""
    want = train_chain(pkg, kind)
    long = engine(pkg, kind, alpha=ALPHA)
    for i, ch in enumerate(chunks(kind)):
        if leg == "train_frames":
            assert ch.train(long) == ch.n // B
        elif leg == "load_then_resident":
            ch.load(long)
            assert long.train_resident(0, ch.n) == ch.n // B
            long.sync()
        else:
            assert ch.train(long, wait=False) == ch.n // B
            continue
        same_bits(state(long), want[i], "call %d ctx %d" % (i, ch.ctx))
    long.sync()
    same_bits(state(long), want[-1], "the end")
    long.close()


@gpu
@pytest.mark.parametrize("kind", ["plain", "nat"])
def test_a_short_chunk_after_a_long_one(pkg, kind):
    """300 frames, then 40 frames of another stream with another table (on each of the two sets): rows of the long
    chunk that lie beyond the short one are never read"""
    nat = kind == "nat"
    big = [Chunk(2, 50 + i, nat, frames=NAT_FRAMES if nat else None) for i in range(2)]
    small = [Chunk(c, 60 + i, nat, nfr=40, frames=[21, 19] if nat else None) for i, c in enumerate((2, 1, 3))]
    long = engine(pkg, kind, alpha=ALPHA)
    for ch in big:
        ch.forward(long)
    for ch in small:
        ref = engine(pkg, kind, alpha=ALPHA)
        assert ch.forward(long).tobytes() == ch.forward(ref).tobytes(), ch.ctx
        assert ch.cv(long).tobytes() == ch.cv(ref).tobytes(), ch.ctx
        ref.close()
    for ch in big:
        ch.forward(long)
    st = state(long)
    for ch in small:
        ref = fresh_from(pkg, kind, st)
        assert ch.train(long) == ch.train(ref) == ch.n // B == 1
        st = state(ref)
        ref.close()
        same_bits(state(long), st, "ctx %d" % ch.ctx)
    long.close()


# ---------------------------------------------------------------------------------------------------------------------
# decoding after a narrow stream
class Decode:
    def __init__(self, kind):
        self.kind, self.nat = kind, kind.endswith("nat")
        self.ls = DEC_NAT_LS if self.nat else DEC_LS
        rng = np.random.default_rng(88 + self.nat)
        nl = len(self.ls) - 1
        self.ws = [rng.normal(0, 0.05, (self.ls[i], self.ls[i + 1])).astype(np.float32) for i in range(nl)]
        self.bs = [rng.normal(0, 0.1, self.ls[i + 1]).astype(np.float32) for i in range(nl)]
        self.mean = rng.normal(10, 2, DD).astype(np.float32)
        self.inv = (1.0 / rng.uniform(2, 4, DD)).astype(np.float32)
        L, S, _ = spec64.params(FS)
        self.waves = [spec64.synth_speech(F * S + L - S + 5 * u, FS, seed=30 + u) for u, F in enumerate(DEC_FRAMES)]
        self.narrow = [self.stream(c, 70 + i) for i, c in enumerate(DEC_NAT_CTX if self.nat else [NARROW_CTX] * 2)]
        self.after = [self.stream(c, 80 + i) for i, c in enumerate(DEC_NAT_CTX if self.nat else [NARROW_CTX])]

    def stream(self, ctx, seed):
        """60 frames of three utterances, 40 samples (some windows twice: context 43 leaves 18 of them)"""
        rng = np.random.default_rng(seed)
        fdim = stream_width(self.ls[0], ctx, self.nat)
        feat = rng.standard_normal((NARROW_FR, fdim)).astype(np.float32)
        targ = rng.standard_normal((NARROW_FR, DD)).astype(np.float32)
        first = rng.integers(0, NARROW_FR - ctx + 1, 40).astype(np.int32)
        tail = ()
        if self.nat:
            fo = [0, 20, 40, NARROW_FR]
            first = np.array([f for f in first if f // 20 == (f + ctx - 1) // 20], np.int32)   # windows inside an utterance
            first = np.resize(first, 40)
            tail = (nat_model.noise_rows(feat, fo, T), nat_model.utt_of_frames(fo, first))
        return (feat, targ, first, ctx, ctx // 2) + tail

    def engine(self, pkg, st=None):
        ws, bs = (self.ws, self.bs) if st is None else (st[:2], st[2:4])
        return engine(pkg, self.kind, ws, bs, ALPHA_D if st is None else st[-1], ls=self.ls, cap=DCAP)

    def load(self, eng, s):
        (eng.load_frames_nat if self.nat else eng.load_frames)(*s)

    def decode(self, eng):
        """(int16, float32) of the first utterance alone, then (int16 list, float32 list, rows) of the batch"""
        one = eng.enhance_wave(self.waves[0], self.mean, self.inv, fea_context=DCTX, fs_khz=FS, return_float=True)
        many = eng.enhance_waves(self.waves, self.mean, self.inv, fs_khz=FS, fea_context=DCTX, return_f32=True,
                                 return_lps=True)
        return one, many


ALPHA_D = np.full(DD, 0.7, np.float32)


@gpu
@pytest.mark.parametrize("kind", ["decode", "decode_nat"])
def test_decoding_after_a_narrow_stream(pkg, kind):
    """load_frames twice (both sets hold rows of 21 floats), then enhance_wave and an enhance_waves call that the chunk
    capacity splits: k_lps_stream / k_lps_stream_seg write rows of 129 floats into those sets.  The waves equal a fresh
    engine's and lie within the float64 chain's bound; a narrow stream afterwards trains as on a fresh engine."""
    dc = Decode(kind)
    assert pkg.enhance_waves_layout([w.size for w in dc.waves], FS)[0].tolist() == DEC_FRAMES
    long = dc.engine(pkg)
    for s in dc.narrow:
        dc.load(long, s)
    one, many = dc.decode(long)
    ref = dc.engine(pkg)
    r_one, r_many = dc.decode(ref)
    slabs = ref.out_slabs()
    ref.close()
    same_bits(one, r_one, "enhance_wave")
    for k in range(3):
        same_bits(many[k], r_many[k], "enhance_waves[%d]" % k)
    same_bits([many[0][0], many[1][0]], one, "the batch's first utterance")
    for u, w in enumerate(dc.waves):
        lps = pkg.wave_to_lps(w, fs_khz=FS)
        z = nat_model.noise_rows(nat_model.normalise(lps, dc.mean, dc.inv), [0, lps.shape[0]], T)[0] if dc.nat else None
        want, eps = spec64.decode64(lps, dc.mean, dc.inv, DCTX, dc.ws, dc.bs, slabs=slabs, nat=z)
        r = spec64.synthesis_ratio(many[1][u], w, want, FS, lps_eps=eps)
        print("%s vs float64: utterance %d ratio %.3g" % (kind, u, r))
        assert r <= 1.0, (u, r)
    st = state(long)
    same_bits(st[:-1], dc.ws + dc.bs, "decoding moved the weights:")
    for s in dc.after:
        ref = dc.engine(pkg, st)
        for e in (long, ref):
            dc.load(e, s)
            assert e.train_resident(0, 40) == 1
            e.sync()
        st = state(ref)
        ref.close()
        same_bits(state(long), st, "ctx %d after decoding" % s[3])
    long.close()


# ---------------------------------------------------------------------------------------------------------------------
# growth is counted: a call that exceeds no capacity makes no device allocation
class Growth:
    """the engine's buffer counter from call to call: bytes held never fall while nothing is closed"""

    def __init__(self, eng):
        self.eng = eng
        self.allocs, self.bytes = eng.buffer_stats()
        assert self.allocs >= 0 and self.bytes >= 0

    def added(self):
        """device allocations since the last look"""
        n, b = self.eng.buffer_stats()
        d, self.allocs = n - self.allocs, n
        assert d >= 0 and b >= self.bytes, (d, b, self.bytes)
        self.bytes = b
        return d


def fresh_forward(pkg, kind, ch):
    ref = engine(pkg, kind, alpha=ALPHA)
    want = ch.forward(ref)
    ref.close()
    return want


@gpu
@pytest.mark.parametrize("kind", ["plain", "nat"])
def test_frames_allocate_only_when_a_capacity_is_exceeded(pkg, kind):
    """the first two calls of the sequence warm the two alternating sets (and chunk_out); a third identical call and a
    shorter stream of the same context allocate nothing; the sequence's first wider row (context 1: 48 or 24 floats a
    row where the sets hold rows of 8) regrows its set.  Every output is a fresh engine's."""
    nat = kind == "nat"
    seq = chunks(kind)
    first, wide = seq[0], seq[2]
    assert wide.fdim > first.fdim and NFR * wide.fdim > (NFR + first.ctx + 8) * first.fdim      # SEQUENCES[kind][2]
    short = Chunk(first.ctx, 90, nat, nfr=44, frames=[23, 21] if nat else None)
    want = fresh_forward(pkg, kind, first)
    long = engine(pkg, kind, alpha=ALPHA)
    g = Growth(long)
    grown = []
    for _ in range(3):
        assert first.forward(long).tobytes() == want.tobytes()
        grown.append(g.added())
    print("%s: allocations of three identical calls %s, %d bytes held" % (kind, grown, g.bytes))
    assert grown[0] >= 1 and grown[1] >= 1 and grown[2] == 0, grown
    assert short.forward(long).tobytes() == fresh_forward(pkg, kind, short).tobytes()
    assert g.added() == 0
    assert wide.forward(long).tobytes() == fresh_forward(pkg, kind, wide).tobytes()
    assert g.added() >= 1
    long.close()


@gpu
@pytest.mark.parametrize("kind", ["decode", "decode_nat"])
def test_decoding_again_allocates_nothing(pkg, kind):
    """enhance_waves on the batch (the chunk capacity splits it: the first call warms both sets), twice more, then its
    first utterance alone through both decoders: no allocation after the first call, every wave a fresh engine's"""
    dc = Decode(kind)
    ref = dc.engine(pkg)
    r_one, r_many = dc.decode(ref)
    ref.close()
    long = dc.engine(pkg)
    g = Growth(long)
    grown = []
    for _ in range(3):
        many = long.enhance_waves(dc.waves, dc.mean, dc.inv, fs_khz=FS, fea_context=DCTX, return_f32=True, return_lps=True)
        for k in range(3):
            same_bits(many[k], r_many[k], "enhance_waves[%d]" % k)
        grown.append(g.added())
    print("%s: allocations of three identical calls %s, %d bytes held" % (kind, grown, g.bytes))
    assert grown[0] >= 1 and grown[1:] == [0, 0], grown
    alone = long.enhance_waves(dc.waves[:1], dc.mean, dc.inv, fs_khz=FS, fea_context=DCTX, return_f32=True, return_lps=True)
    for k in range(3):
        same_bits(alone[k], r_many[k][:1], "alone[%d]" % k)
    assert g.added() == 0
    # (enhance_wave borrows the raw sets and chunk_out; its other buffers live for the call and are not counted)
    same_bits(long.enhance_wave(dc.waves[0], dc.mean, dc.inv, fea_context=DCTX, fs_khz=FS, return_float=True), r_one,
              "enhance_wave")
    assert g.added() == 0
    long.close()


LIVE_K = 103                                             # a block of 128 (K + 1) samples: see the test below


@gpu
def test_a_second_live_push_allocates_nothing(pkg):
    """Two sessions, two pushes of 128 (K + 1) = 13312 samples each, the second ending both.  At 8 kHz (frames of 256
    samples every 128, 3 frames of look-ahead) the first push decodes K - 3 = 100 frames a session, the second K + 4 =
    107: by the chunk capacity of 64 that is four chunks either time, the one chunk that touches both sessions (76
    stream rows, the most a chunk can have) is the second either time and, four being even, lands on the same raw set;
    the group's per-push workspaces grow by less than their eighth of headroom.  So the second push allocates nothing.
    The group's buffers are counted ON THE ENGINE (mlggd_debug_buffers): the allocation count stays where it is when
    the group closes, the bytes fall by what the group held.  What the sessions emitted is enhance_wave of the whole
    recording on a fresh engine."""
    dc = Decode("decode")
    n = 128 * (LIVE_K + 1)
    waves = [spec64.synth_speech(2 * n, FS, seed=40 + u) for u in range(2)]
    ref = dc.engine(pkg)
    want = [ref.enhance_wave(w, dc.mean, dc.inv, fea_context=DCTX, fs_khz=FS) for w in waves]
    ref.close()
    long = dc.engine(pkg)
    g = Growth(long)
    before = g.bytes
    grp = long.live(dc.mean, dc.inv, 2, fs_khz=FS, fea_context=DCTX)
    opened = g.added()
    out1 = grp.push([w[:n] for w in waves])
    pushed = g.added()
    assert [o.size for o in out1] == [128 * (LIVE_K - 3)] * 2
    out2 = grp.push([w[n:] for w in waves], end=[True, True])
    again = g.added()
    print("live: allocations at open %d, first push %d, second push %d, %d bytes held" % (opened, pushed, again, g.bytes))
    assert opened >= 1 and pushed >= 1 and again == 0
    for u in range(2):
        got = np.concatenate([out1[u], out2[u]])
        assert got.dtype == want[u].dtype and got.tobytes() == want[u].tobytes(), u
    held, count = g.bytes, g.allocs
    grp.close()
    n_after, b_after = long.buffer_stats()
    assert n_after == count and before < b_after < held, (n_after, count, before, b_after, held)
    long.close()
