"""The set-switching loop (bank::set_loop, forward_bank.hpp) through each of the seven kernels it serves:
one table of item lists, every list run through every entry that can express it.

An item is a window of T samples of one of four sample streams under one of three sets; its reference
row, logits and layer-4 features, is the C oracle of that set on the materialised window
(support_features.features, computed once per window and set), never a GPU entry.  A list is a
sequence of tokens: a set index (a valid item under that set), INV (an invalid item: a zero row, a zero
feature row and one count in n_bad) and ABS (an each-group's absent item: its row is not written).
Every output buffer is prefilled, so a row nobody wrote shows; every row, every feature row and n_bad
are compared exactly.  Grid caps 1 and 2: one workgroup walks the list, or the two ranges
range_of(w, 2, n) do, so that the boundary falls inside it.

What the lists hold (LISTS):
  1. the first item of a range invalid, the next valid under set 0 (no switch follows the load of set 0)
  2. the first item invalid, the next valid under set 2
  3. valid(a) -> valid(b): item i - 1 is finished on set a
  4. valid(a) -> invalid -> valid(b): the invalid item's zero row and count are written at the switch
  5. the last item of a range invalid; the last item of a range valid right after a switch
  6. each-groups (INV read as ABS): an absent session between two sessions of different sets, at the
     start and at the end of a range, and a whole range of absent items
  7. the _feat entries: an invalid item's feature row is zeros, at T64 = 1 (bytes) and T64 = 4 (16-byte rows)

How an entry makes an item invalid: an onset or a set index out of range (epochs through a bank); a
window that straddles two sets, or a gap (windows through a bank); an onset before the origin after
net_streams_restart (the uniform push); a session index out of range or an onset outside the retained
span (queries).  test_inputs_tell_the_sets_apart needs no GPU: it certifies that a row finished on a
neighbour's set would show.
"""
import functools

import numpy as np
import pytest

import support_features as sf
from mibminet import lib
from mibminet.params import ParamSet

INV, ABS = "x", "-"
# 5 x 100, N = 3: T64 = 1, features leave as bytes, T mod 16 != 0.  8 x 256, N = 2: T64 = 4, the 16-byte path.
SHAPES = [(5, 100, 3), (8, 256, 2)]
# REORDER_BN with the float requant, and plain BN with exact division: whichever flag the kernels share
# decides whether T is held or read per window
FLAVOURS = ["reorder-float", "plain-exact"]
CAPS = (1, 2)
LISTS = {
    # cap 1: 1, 3, 4, an invalid item between two of one set, the last invalid.  cap 2: the first range ends
    # valid right after a switch, the second starts invalid and goes on under set 2 and ends invalid
    "a": (INV, 0, 0, 1, INV, 2, INV, 2, 1, 1, 0, INV),
    # cap 1: 2, runs of invalid items, the last item valid right after a switch.  cap 2: both ranges too
    "b": (INV, 2, INV, INV, 0, 1, 2, INV, 0, 2, INV, 1),
    # cap 2: a whole range of invalid (absent) items after a range that ends on them
    "c": (1, 1, 1, INV, INV, INV, INV, INV, INV, INV, INV, INV),
    # an odd count: the ranges of cap 2 are [0, 2) and [2, 5)
    "d": (2, INV, 0, INV, 1),
}
STREAMS, SPAN, TAIL = 4, 41, 3  # the streams, the onsets 0 .. SPAN - 1 of an item, the samples past the last window
FILL = 0x55


def n_of(T):
    """The samples of a session's second push: with the LEAD before them the position is T + TAIL, and
    with hop n_of(T) exactly window 0 ends in it."""
    return T + TAIL - LEAD


LEAD = 8  # the samples of a session's first push, which completes no window; a restart then sets the origin to 8


@functools.lru_cache(maxsize=None)
def sets_of(C, T, N, flavour):
    if flavour == "reorder-float":
        return tuple(ParamSet.synthetic(seed=311 + s, C=C, T=T, N=N) for s in range(3))
    return tuple(ParamSet.synthetic_extreme(seed=321 + s, C=C, T=T, N=N, mids=3, reorder_bn=False) for s in range(3))


@functools.lru_cache(maxsize=None)
def streams_of(C, T):
    x = np.random.default_rng([C, T, 83]).integers(-127, 128, size=(STREAMS, C, SPAN + T + TAIL), dtype=np.int8)
    x.setflags(write=False)
    return x


def items_of(tokens):
    """[(stream, onset, set) or None]: item k of a list.  A set's items come from the stream of its own
    index, those of set 1 in turn from stream 3 too, which the query groups hold under set 1 as well."""
    out = []
    for k, t in enumerate(tokens):
        out.append(None if t in (INV, ABS) else (3 if t == 1 and k % 2 else t, (7 * k + 3) % SPAN, t))
    return out


_ROWS = {}


def reference(C, T, N, flavour, tokens, absent=False):
    """(logits [n][N], features [n][16 T64]) of a list: the oracle's rows of its valid items, zeros for
    an invalid item or, `absent`, the prefill."""
    sets, x = sets_of(C, T, N, flavour), streams_of(C, T)
    T64 = T // 64
    y = np.full((len(tokens), N), FILL if absent else 0, np.int8)
    f = np.full((len(tokens), 16 * T64), FILL if absent else 0, np.int8)
    for k, it in enumerate(items_of(tokens)):
        if it is None:
            continue
        key = (C, T, N, flavour) + it
        if key not in _ROWS:
            i, o, s = it
            feat, logits = sf.features(sets[s], np.ascontiguousarray(x[i][None, :, o: o + T]))
            _ROWS[key] = (logits[0], feat[0].reshape(-1))
        y[k], f[k] = _ROWS[key]
    return y, f


# ---- the entries: tokens -> (logits [n][N], features or None, n_bad) --------------------------------
class Ctx:
    def __init__(self, torch, bank, C, T, N, flavour):
        self.torch, self.bank, self.C, self.T, self.N, self.flavour = torch, bank, C, T, N, flavour
        self.x = streams_of(C, T)
        self.fb = 16 * (T // 64)

    def out(self, n):
        t = self.torch
        return (t.full((n, self.N), FILL, dtype=t.int8, device="cuda"), t.full((n, self.fb), FILL, dtype=t.int8, device="cuda"),
                t.zeros((1,), dtype=t.int32, device="cuda"))

    def done(self, rc, y, f, nb):
        assert rc == lib.NET_OK, rc
        self.torch.cuda.synchronize()
        return y.cpu().numpy(), None if f is None else f.cpu().numpy(), int(nb.item())

    def dev(self, v, dtype):
        return self.torch.tensor([int(a) for a in v], dtype=dtype, device="cuda")


def epochs_bank(cx, tokens, feat):
    """The streams as one source [STREAMS C][L]; item (i, o) is the epoch at element i C L + o.  An
    invalid item is in turn an onset past the last valid one, a negative onset, set index 3 and set
    index -1 (on a valid onset)."""
    t, L = cx.torch, cx.x.shape[2]
    src = t.from_numpy(cx.x.reshape(STREAMS * cx.C, L).copy()).cuda()
    last = src.numel() - ((cx.C - 1) * L + cx.T)
    onsets, set_of, bad = [], [], 0
    for it in items_of(tokens):
        if it is None:
            onsets.append((last + 1, -1, 5, 5)[bad % 4])
            set_of.append((0, 1, 3, -1)[bad % 4])
            bad += 1
        else:
            onsets.append(it[0] * cx.C * L + it[1])
            set_of.append(it[2])
    y, f, nb = cx.out(len(tokens))
    ond, sod = cx.dev(onsets, t.int64), cx.dev(set_of, t.int32)
    lead = (cx.bank.handle, src.data_ptr(), src.numel(), L, None, ond.data_ptr(), sod.data_ptr(), len(tokens), y.data_ptr())
    if feat:
        return cx.done(lib.load().net_model_compute_epochs_bank_feat(*lead, f.data_ptr(), nb.data_ptr(), 0, None), y, f, nb)
    return cx.done(lib.load().net_model_compute_epochs_bank(*lead, nb.data_ptr(), 0, None), y, None, nb)


def windows_bank(cx, tokens):
    """One region of 16 ceil(T / 16) samples per item, laid along time, its blocks under the item's
    set and its window at its start.  An invalid item's region is in turn one whose last block has
    another set (the window straddles two sets) and a gap."""
    t, T = cx.torch, cx.T
    R = (T + 15) // 16 * 16
    n = len(tokens)
    xs = np.zeros((cx.C, n * R), np.int8)
    blk = np.zeros(n * R // 16, np.int32)
    bad = 0
    for k, it in enumerate(items_of(tokens)):
        b = slice(k * R // 16, (k + 1) * R // 16)
        if it is None:
            xs[:, k * R: k * R + T] = cx.x[0][:, :T]
            blk[b] = 0 if bad % 2 == 0 else -1
            if bad % 2 == 0:
                blk[b.stop - 1] = 1
            bad += 1
        else:
            xs[:, k * R: k * R + T] = cx.x[it[0]][:, it[1]: it[1] + T]
            blk[b] = it[2]
    L = n * R
    xd, bd = t.from_numpy(xs).cuda(), t.from_numpy(blk).cuda()
    ond = cx.dev([k * R for k in range(n)], t.int64)
    wsb = lib.load().net_windows_workspace(L)
    ws = t.empty((wsb,), dtype=t.int8, device="cuda")
    y, _, nb = cx.out(n)
    rc = lib.load().net_model_compute_windows_bank(cx.bank.handle, xd.data_ptr(), 1, L, bd.data_ptr(), ond.data_ptr(), n,
                                                   y.data_ptr(), nb.data_ptr(), ws.data_ptr(), wsb, 0, None)
    return cx.done(rc, y, None, nb)


def _session_chunks(cx, tokens):
    """[n][C][T + TAIL]: session k's samples, its item's window from sample 0 (an item without one: stream 0's)."""
    return np.stack([cx.x[it[0] if it else 0][:, (it[1] if it else 0):][:, : cx.T + TAIL] for it in items_of(tokens)])


def push(cx, tokens):
    """One session per item under the item's set, hop n_of(T): a push of LEAD samples, a restart of the
    invalid items' sessions (their origin is then LEAD, past window 0's onset), and the push whose one
    window per session is the item."""
    t = cx.torch
    its = items_of(tokens)
    xs = t.from_numpy(_session_chunks(cx, tokens)).cuda()
    n = n_of(cx.T)
    with lib.Streams(cx.bank, [it[2] if it else 1 for it in its], n, n) as g:
        g.push(xs[:, :, :LEAD].contiguous())
        for k, it in enumerate(its):
            if it is None:
                g.restart(k, k % 3)
        assert g.windows(n) == 1
        x2 = xs[:, :, LEAD:].contiguous()
        y, _, nb = cx.out(len(tokens))
        rc = lib.load().net_streams_push(g.handle, x2.data_ptr(), 1, n, y.data_ptr(), nb.data_ptr(), None)
        return cx.done(rc, y, None, nb)


def push_each(cx, tokens):
    """push's sessions in an each-group: every session LEAD samples, then the present items' sessions
    n_of(T) more, which completes their window 0, and the absent items' sessions in turn none and TAIL."""
    t = cx.torch
    its = items_of(tokens)
    xs = t.from_numpy(_session_chunks(cx, tokens)).cuda()
    n = n_of(cx.T)
    with lib.StreamsEach(cx.bank, [it[2] if it else 1 for it in its], n, n) as g:
        assert g.rows(n) == 1
        slot = t.zeros((len(its), cx.C, n), dtype=t.int8, device="cuda")
        slot[:, :, :LEAD] = xs[:, :, :LEAD]
        g.push(slot, t.full((len(its),), LEAD, dtype=t.int32, device="cuda"))
        counts = [n if it else (0, TAIL)[k % 2] for k, it in enumerate(its)]
        slot.copy_(xs[:, :, LEAD:])
        y, _, nb = cx.out(len(tokens))
        cout = t.zeros((len(its),), dtype=t.int32, device="cuda")
        cin = cx.dev(counts, t.int32)
        rc = lib.load().net_streams_push_each(g.handle, slot.data_ptr(), 1, cin.data_ptr(), n, y.data_ptr(), cout.data_ptr(),
                                              None, nb.data_ptr(), None)
        got = cx.done(rc, y, None, nb)
        assert cout.cpu().tolist() == [1 if it else 0 for it in its]
        return got


QUERY_SETS = (0, 1, 2, 1)  # the set of stream i's session in the query groups


def windows_at(cx, tokens, feat, each):
    """A group of the four streams' sessions, every sample pushed (the ring keeps them all: the span is
    0 .. SPAN + TAIL - 1); item (i, o) is the query (session i, onset o).  An invalid item is in turn
    session STREAMS, session -1, an onset one past the newest window's and onset -1."""
    t, T = cx.torch, cx.T
    total = cx.x.shape[2]
    xs = t.from_numpy(cx.x.copy()).cuda()
    max_push = (total + 1) // 2
    ses, ons, bad = [], [], 0
    for it in items_of(tokens):
        if it is None:
            ses.append((STREAMS, -1, 1, 2)[bad % 4])
            ons.append((0, 0, total - T + 1, -1)[bad % 4])
            bad += 1
        else:
            assert QUERY_SETS[it[0]] == it[2]
            ses.append(it[0])
            ons.append(it[1])
    with (lib.StreamsEach if each else lib.Streams)(cx.bank, QUERY_SETS, 1 << 20, max_push) as g:
        assert g.cap >= total
        for lo in range(0, total, max_push):
            chunk = xs[:, :, lo: lo + max_push]
            if each:
                slot = t.zeros((STREAMS, cx.C, max_push), dtype=t.int8, device="cuda")
                slot[:, :, : chunk.shape[2]] = chunk
                g.push(slot, t.full((STREAMS,), chunk.shape[2], dtype=t.int32, device="cuda"))
            else:
                g.push(chunk.contiguous())
        y, f, nb = cx.out(len(tokens))
        sd, od = cx.dev(ses, t.int32), cx.dev(ons, t.int64)
        lead = (g.handle, sd.data_ptr(), od.data_ptr(), len(tokens), y.data_ptr())
        if feat:
            return cx.done(lib.load().net_streams_windows_at_feat(*lead, f.data_ptr(), nb.data_ptr(), None), y, f, nb)
        return cx.done(lib.load().net_streams_windows_at(*lead, nb.data_ptr(), None), y, None, nb)


# name: (the call, the kernel it runs, whether an item without a window is absent)
ENTRIES = {
    "epochs_bank": (lambda cx, tk: epochs_bank(cx, tk, False), "bank::k_forward_ep_bank", False),
    "epochs_bank_feat": (lambda cx, tk: epochs_bank(cx, tk, True), "bank::k_forward_ep_bank_feat", False),
    "windows_bank": (windows_bank, "bank::k_forward_y1_bank", False),
    "push": (push, "stream::k_forward_ring", False),
    "push_each": (push_each, "stream::k_forward_ring_each", True),
    "windows_at": (lambda cx, tk: windows_at(cx, tk, False, False), "stream::k_forward_ring_at", False),
    "windows_at_each": (lambda cx, tk: windows_at(cx, tk, False, True), "stream::k_forward_ring_at (each-group)", False),
    "windows_at_feat": (lambda cx, tk: windows_at(cx, tk, True, False), "stream::k_forward_ring_at_feat", False),
    "windows_at_feat_each": (lambda cx, tk: windows_at(cx, tk, True, True), "stream::k_forward_ring_at_feat (each-group)", False),
}


@pytest.fixture(scope="module")
def banks(gpu):
    cache = {}

    def get(C, T, N, flavour):
        key = (C, T, N, flavour)
        if key not in cache:
            cache[key] = lib.Bank(sets_of(*key))
            assert cache[key].exact_division == (flavour == "plain-exact")
        return cache[key]

    yield get
    for b in cache.values():
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("C,T,N", SHAPES)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_transition(gpu, banks, entry, C, T, N, flavour):
    import torch

    call, kernel, absent = ENTRIES[entry]
    cx = Ctx(torch, banks(C, T, N, flavour), C, T, N, flavour)
    try:
        for name, tokens in LISTS.items():
            want_y, want_f = reference(C, T, N, flavour, tokens, absent)
            want_bad = 0 if absent else sum(t == INV for t in tokens)
            for cap in CAPS:
                lib.grid_cap(cap)
                y, f, n_bad = call(cx, tokens)
                what = f"{kernel}, list {name}, grid cap {cap}"
                rows = np.flatnonzero((y != want_y).any(1))
                assert rows.size == 0, f"{what}: logit rows {rows.tolist()} differ"
                if f is not None:
                    rows = np.flatnonzero((f != want_f).any(1))
                    assert rows.size == 0, f"{what}: feature rows {rows.tolist()} differ"
                assert n_bad == want_bad, f"{what}: n_bad {n_bad}, expected {want_bad}"
    finally:
        lib.grid_cap(0)


def test_inputs_tell_the_sets_apart():
    """(No GPU.)  What the comparisons above rest on: no reference row is all zeros or all prefill, and a window's
    rows under the three sets differ pairwise, so an item finished on a neighbour's set shows."""
    for C, T, N in SHAPES:
        for flavour in FLAVOURS:
            for s in range(3):
                y, f = reference(C, T, N, flavour, tuple([s] * 12))
                assert y.any(1).all() and f.any(1).all() and (y != FILL).any(1).all()
            rows = []
            for s in range(3):  # the same twelve windows under each set
                sets, x = sets_of(C, T, N, flavour), streams_of(C, T)
                wins = np.stack([x[k % STREAMS][:, (7 * k + 3) % SPAN:][:, :T] for k in range(12)])
                rows.append(sf.features(sets[s], wins))
            for a in range(3):
                for b in range(a + 1, 3):
                    assert (rows[a][1] != rows[b][1]).any(1).all() and (rows[a][0] != rows[b][0]).any((1, 2)).all()
