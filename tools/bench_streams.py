#!/usr/bin/env python3
"""One tick of many live sessions: a push into the sessions' layer-1 rings against the chunking
recipe a caller had before.

For each case (one MI355X, one process, HIP events around each candidate, host work included), every
session receives n new samples per tick:
  (a) one net_streams_push over all sessions: layer 1 on the n new samples, then the windows that
      end in them out of the rings;
  (b) one net_model_compute_windows_bank call on the S overlapped chunks [C][T - hop + n] (the last
      T - hop samples a caller keeps per session, then the n new ones) laid at multiples of 16
      samples: layer 1 runs again on every kept sample.  The array, its block list and its onsets are
      prepared outside the timed region, which flatters (b): a caller rebuilds the array every tick.
  (l) (a)'s first phase alone: a push into a second group whose hop no window ever meets, so that
      only the layer-1 kernel is enqueued; (a) - (l) is what the windows kernel and its launch add.
The sessions are int8, hop 8, session i under set sets[i] of one bank.  First the rings are filled
and a few ticks are run through both on the same samples: every logit row of (a) must equal (b)'s.
Then a, b and l alternate within every warm-up round and every timed repeat; the medians and maxima
over --reps ticks are reported.  The only gate is a < b on the medians.  One JSON line per case goes
to <out-dir>/streams_<name>.json and to stdout.  There is no CPU path.

Sessions at their own pace (net_streams_push_each), in the same process and on the same sessions as
bci_1024 (1,024 of 22 x 1125 under 16 sets, grouped, hop 8):
  each_equal   every count 16 = n_max.  (e) net_streams_push_each against (u) net_streams_push of a
               uniform group on the same samples: the reference is the uniform push, and e / u is
               what the plan launch and the record loads cost.  Verified first: over six ticks every
               row of (e) equals (u)'s.
  each_ragged  counts drawn uniformly from 0 .. 32 = n_max (mean 16).  (e) against (b) the chunking
               recipe, the only way to serve ragged sessions before: one net_model_compute_windows_bank
               call on the sessions' kept samples followed by their new ones (session i from the onset
               of its first window that ends in the tick, nothing for a session that completes none),
               laid at multiples of 16 samples, the array and its lists prepared outside the timed
               region, which flatters (b).  Verified first: every completed row of (e) equals (b)'s.
In both, (e) is also captured into a graph once and replayed, (g).  Two timing rounds of their own:
e alternating with its reference, no replay anywhere near them, gives e / reference; then e
alternating with g gives g / e (that round's e is reported as *_beside_graph).  Per candidate two
times are kept apart: the device's (HIP events around the call) and the host's (a clock around the
enqueue alone, the queue drained before it).  No gate on these times: nothing here had been
measured before.

Float32 frames as an amplifier delivers them (net_streams_push_f32_tm), 1,024 sessions under 16 sets,
hop 8, n 16, each candidate with a stream group of its own fed the same samples:
  f32_tm          22 x 1125.  (new) net_streams_push_f32_tm on [S][n][C]; (a) what a caller did before: a
                  torch transpose of the tick's frames to [S][C][n] and net_streams_push_f32, both inside
                  the timed region; (b) net_streams_push_f32 alone on frames transposed outside it.  The
                  claim checked is new <= a ((a) is an extra pass over the same data, then the same
                  work); (b) is reported, not judged.
  f32_tm_montage  19 of 64 electrodes, 19 x 1125.  (new) net_streams_push_f32_tm on [S][n][64] through sets
                  widened to 64 rows (net_blob_widen); (a) index_select of the 19 columns, the transpose
                  and net_streams_push_f32 through the original sets, all timed; (b) as above.  One
                  channel map serves every session here, which flatters (a): index_select cannot apply a
                  map per session.
Verified first in both: over six ticks every logit row of (new) equals (a)'s and (b)'s.  The three
alternate within every warm-up round and every timed repeat.

Frames at the amplifier's own rate (net_streams_push_raw_f32_tm), 1,024 sessions of 22 x 1125 under 16
grouped sets, hop 8, 16 decimated samples per tick, i.e. 16 q raw float32 frames [S][16 q][C]:
  f32_tm_decim    Two settings, q = 2 with K = 41 taps and q = 4 with K = 81 (decimate.firwin_taps), each with
                  three stream groups fed the same frames.  (new) net_streams_push_raw_f32_tm: the FIR inside
                  the layer-1 kernel, the histories on the device; (a) the caller's recipe, all timed: a kept
                  tail of K - 1 frames, torch.cat, a strided depthwise conv1d, the transpose back to frames
                  and net_streams_push_f32_tm; (b) net_streams_push_f32_tm alone on frames decimated
                  beforehand.  The rings are filled with zero frames; then over six ticks of random frames
                  every row of (new) must equal (b)'s on decimate.fir_decimate's samples (the CPU's, bit
                  for bit what the kernel computes); (a)'s float sums are the convolution library's and its
                  rows are compared for the record only.  The claim checked is new <= a on the medians, with no
                  margin; new / b is reported, not judged.

Raw frames at each session's own pace (net_streams_push_each_raw_f32_tm), 1,024 sessions of 22 x 1125
under 16 grouped sets, hop 8, with (q, K) = (2, 41) and (4, 81) from decimate.firwin_taps; the rings are
filled with zero frames at equal counts, then six ticks of random frames are verified, then timed:
  each_raw_equal  every count 16 q = n_raw_max.  (new) net_streams_push_each_raw_f32_tm against (u)
                  net_streams_push_raw_f32_tm of a uniform group on the same frames (new / u is what
                  the plan launch and the two records cost: set it beside each_equal's e / u from the
                  same run) and against (b) net_streams_push_each_f32_tm on frames decimated beforehand.
                  Verified first: every row of (new) equals (u)'s and (b)'s on decimate.fir_decimate's
                  samples.  Report only.
  each_raw_ragged counts drawn uniformly from 0 .. 32 q = n_raw_max.  (new) against (a) the caller's
                  recipe, all timed: per-session kept tails of K - 1 frames, torch.cat, a stride-1
                  depthwise conv1d over tail plus slot, a gather of each session's phase (and of its
                  new tail), the positions' arithmetic on the device, then
                  net_streams_push_each_f32_tm; and (b) as above.  Verified first: every completed
                  row of (new) equals (b)'s on the CPU's samples, session by session; (a)'s float sums
                  are the convolution library's and its rows are compared for the record only.  The
                  claim checked is new <= a on the medians, with no margin.
In both, (new) is also captured into a graph once and replayed, (g), in a round of its own beside
the eager call, as each_equal does.

An IIR prefilter ahead of the decimator (net_streams_set_prefilter), 1,024 sessions of 22 x 1125 under
16 grouped sets, hop 8, 16 decimated samples per tick, (q, K) = (2, 41) and (4, 81); the prefilter is
M = 3: decimate.butter_sos(4, 0.5 Hz, high-pass) plus decimate.biquad("notch", 50 Hz, Q 30) at
fs = 250 q; the frames are unit noise on a DC offset of 100:
  f32_tm_prefilter    a uniform group.  (new) net_streams_push_raw_f32_tm with the prefilter; (p) the
                      same push on a twin group without one and the same frames (new - p is what the
                      prefilter costs per tick: recorded, not bounded); (a) the caller's recipe, all
                      timed: the same recursion frame by frame in torch ops on [S][C] device tensors
                      with carried state, then the raw push of the result.  Verified first, from zero
                      state until past the first windows: every completed row of (new) equals (p)'s on
                      decimate.sos_filter's frames (the CPU's, bit for bit the contract).  The claim
                      checked is new <= a on the medians, with no margin, in every setting of both
                      cases: the tool exits non-zero where it fails.
  each_raw_prefilter  the same on an each-group, once with every count n_raw_max and once with counts
                      drawn uniformly from 0 .. n_raw_max ((a) then masks its state updates per
                      session), and (new) captured into a graph and replayed beside its eager call.

Cue-locked trials of live sessions (net_streams_windows_at), 1,024 sessions of 22 x 1125 under 16
grouped sets, hop 8, n 16:
  at_cues         Every tick is a push followed by one query per session, at an onset drawn uniformly
                  inside the session's span of cap - T + 1 onsets, the items sorted by session.  (new)
                  net_streams_windows_at: layers 2-5 on rows read out of the rings; (b) what a caller ran
                  before: net_model_compute_epochs_bank on the same onsets over a raw-sample array
                  [S][C][cap] of every session's last cap samples, which runs layer 1 on T samples per
                  window.  The array is prepared outside the timed region, which flatters (b): a caller
                  rewrites it every tick.  (g) a hop-1 group's grid rows cover a cue only at hop times
                  the layers 2-5 work of every push, for windows nobody reads: said, not timed.
                  Verified first: over six ticks every row of (new) equals (b)'s.  Then per tick the push
                  is timed on its own and (new) and (b) take turns going first; the only claim is
                  new <= b on the medians.
  at_feat         (report only, no gate) at_cues' sessions, pushes and cues: per tick (new)
                  net_streams_windows_at, (new2) the same call again, so that the run-to-run spread of
                  one candidate stands beside the numbers, and (feat) net_streams_windows_at_feat, which
                  also stores 16 T64 bytes of layer-4 activations per window; the three rotate their
                  order from tick to tick.  Verified first: over six ticks (feat)'s logits equal (new)'s.

  python tools/bench_streams.py [--cases mmmi_64,bci_1024,bci_1024_shuffled,each_equal,each_ragged,f32_tm,f32_tm_montage,f32_tm_decim,each_raw_equal,each_raw_ragged,f32_tm_prefilter,each_raw_prefilter,at_cues,at_feat]
                                [--limit S] [--reps 1000] [--warmup 50] [--variant canonical|plain_bn]
                                [--out-dir profiles]
"""
import statistics
import time

from bench_common import main, medians, min_max, time_alternating

HOP = 8
VERIFY = 6  # ticks run through both candidates on the same samples
CASES = {  # name: (sessions, sets, C, T, N, n, sets shuffled over the sessions)
    "mmmi_64": (64, 64, 64, 480, 2, 8, False),
    "bci_1024": (1024, 16, 22, 1125, 4, 16, False),
    "bci_1024_shuffled": (1024, 16, 22, 1125, 4, 16, True),
}
EACH_CASES = {  # name: (sessions, sets, C, T, N, n_max, counts drawn from 0 .. n_max): net_streams_push_each
    "each_equal": (1024, 16, 22, 1125, 4, 16, False),
    "each_ragged": (1024, 16, 22, 1125, 4, 32, True),
}
F32_CASES = {  # name: (sessions, sets, C, T, N, n, source rows R): net_streams_push_f32_tm
    "f32_tm": (1024, 16, 22, 1125, 4, 16, 22),
    "f32_tm_montage": (1024, 16, 19, 1125, 4, 16, 64),
}
DECIM_CASES = {  # name: (sessions, sets, C, T, N, decimated samples per tick, ((q, K), ...)): net_streams_push_raw_f32_tm
    "f32_tm_decim": (1024, 16, 22, 1125, 4, 16, ((2, 41), (4, 81))),
}
EACH_RAW_CASES = {  # name: (sessions, sets, C, T, N, most decimated samples per tick, ragged, ((q, K), ...))
    "each_raw_equal": (1024, 16, 22, 1125, 4, 16, False, ((2, 41), (4, 81))),
    "each_raw_ragged": (1024, 16, 22, 1125, 4, 32, True, ((2, 41), (4, 81))),
}

PREFILTER_CASES = {  # name: (sessions, sets, C, T, N, decimated samples per tick, each-group, ((q, K), ...))
    "f32_tm_prefilter": (1024, 16, 22, 1125, 4, 16, False, ((2, 41), (4, 81))),
    "each_raw_prefilter": (1024, 16, 22, 1125, 4, 16, True, ((2, 41), (4, 81))),
}
AT_CASES = {  # name: (sessions, sets, C, T, N, n): net_streams_windows_at
    "at_cues": (1024, 16, 22, 1125, 4, 16),
}
AT_FEAT_CASES = {  # name: (sessions, sets, C, T, N, n): net_streams_windows_at_feat beside net_streams_windows_at
    "at_feat": (1024, 16, 22, 1125, 4, 16),
}


def run_case(name, limit, reps, warmup, variant, seed=2026):
    if name in AT_CASES:
        return run_at(name, limit, reps, warmup, variant, seed)
    if name in AT_FEAT_CASES:
        return run_at_feat(name, limit, reps, warmup, variant, seed)
    if name in EACH_CASES:
        return run_each(name, limit, reps, warmup, variant, seed)
    if name in F32_CASES:
        return run_f32(name, limit, reps, warmup, variant, seed)
    if name in DECIM_CASES:
        return run_decim(name, limit, reps, warmup, variant, seed)
    if name in EACH_RAW_CASES:
        return run_each_raw(name, limit, reps, warmup, variant, seed)
    if name in PREFILTER_CASES:
        return run_prefilter(name, limit, reps, warmup, variant, seed)
    import numpy as np
    import torch

    from mibminet import lib
    from mibminet.params import ParamSet

    S, n_sets, C, T, N, n, shuffled = CASES[name]
    S = min(S, limit)  # --limit: fewer sessions, for a quick look
    n_sets = min(n_sets, S)
    sets = [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(n_sets)]
    bank = lib.Bank(sets)
    set_of = np.sort(np.arange(S) * n_sets // S)  # grouped by set
    if shuffled:
        set_of = np.random.default_rng(seed).permutation(set_of)
    set_of = [int(v) for v in set_of]
    st = lib.Streams(bank, set_of, HOP, n)
    st_l1 = lib.Streams(bank, set_of, 2**40, n)  # (l): no window ends in any push
    k = n // HOP  # windows per session and tick once the position is T mod hop
    Lc = T - HOP + n
    # the first push brings the position to T mod hop, so that every later one of n samples ends on the grid
    lead = T % HOP
    fill = -(-(T - lead) // n)  # pushes of n until the first window
    total = lead + (fill + VERIFY) * n
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-128, 128, (S, C, total), dtype=torch.int8, device="cuda", generator=g)
    # (b)'s layout: session i's chunk at sample i stride of one array [C][Lx]
    starts, Lx, blk_set, onsets, first = lib.bank_windows_lists(bank, [Lc] * S, set_of, HOP)
    assert len(onsets) == S * k and Lx * max(16, C) < 2**31
    stride = int(starts[1]) if S > 1 else Lc
    xb = torch.zeros((C, Lx), dtype=torch.int8, device="cuda")
    lay = torch.zeros((C, S, stride), dtype=torch.int8, device="cuda")  # the chunks at their starts, pads zero
    ond, bsd = torch.from_numpy(onsets).cuda(), torch.from_numpy(blk_set).cuda()
    wsb = lib.windows_workspace(Lx)
    ws = torch.empty((wsb,), dtype=torch.int8, device="cuda")
    ya, yb, yl = (torch.empty((S, k, N), dtype=torch.int8, device="cuda") for _ in range(3))
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")
    A = lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    xa = x[:, :, :n].contiguous()

    def a():
        rc = A.net_streams_push(st.handle, xa.data_ptr(), 1, n, ya.data_ptr(), nbad.data_ptr(), stream)
        assert rc == 0, rc

    def b():
        rc = A.net_model_compute_windows_bank(bank.handle, xb.data_ptr(), 1, Lx, bsd.data_ptr(), ond.data_ptr(), S * k,
                                              yb.data_ptr(), nbad.data_ptr(), ws.data_ptr(), wsb, 0, stream)
        assert rc == 0, rc

    def l():
        # (window 0 ends in one push of the run, whatever the hop: that one writes its rows to yl)
        rc = A.net_streams_push(st_l1.handle, xa.data_ptr(), 1, n, yl.data_ptr(), None, stream)
        assert rc == 0, rc

    # fill the rings, then VERIFY ticks through both on the same samples
    pos = 0
    for m in [lead] * (lead > 0) + [n] * fill:
        y, _ = st.push(x[:, :, pos: pos + m].contiguous())
        pos += m
    assert st.windows(n) == k and pos % HOP == T % HOP
    mis = 0
    for _ in range(VERIFY):
        xa.copy_(x[:, :, pos: pos + n])
        # session i's last Lc samples at columns i stride .. i stride + Lc - 1
        lay[:, :, :Lc].copy_(x[:, :, pos + n - Lc: pos + n].transpose(0, 1))
        xb.copy_(lay.view(C, S * stride)[:, :Lx])
        a()
        b()
        pos += n
        torch.cuda.synchronize()
        mis += int((ya != yb).any(dim=2).sum().item())
    assert int(nbad.item()) == 0
    info = bank.info()
    res = {"name": name, "sessions": S, "sets": n_sets, "shuffled": shuffled, "C": C, "T": T, "N": N, "hop": HOP, "n": n,
           "windows_per_tick": S * k, "ring_samples": st.cap, "ring_bytes": S * 32 * st.cap,
           "chunk_samples_b": Lc, "layer1_samples_b_over_a": round(Lc / n, 2), "variant": variant,
           "exact_division": bool(info[4]), "verified_ticks": VERIFY, "mismatched_rows": mis, "reps": reps,
           "warmup": warmup, "device": torch.cuda.get_device_name(0)}
    ms = time_alternating({"a": a, "b": b, "l": l}, reps, warmup)
    med = medians(ms)
    res.update({"ms_push": round(med["a"], 4), "ms_chunked_windows_bank": round(med["b"], 4),
                "ms_push_layer1_only": round(med["l"], 4),
                "ms_push_min_max": min_max(ms["a"]), "ms_chunked_windows_bank_min_max": min_max(ms["b"]),
                "ms_push_layer1_only_min_max": min_max(ms["l"]),
                "a_over_b": round(med["a"] / med["b"], 4), "windows_per_s": round(S * k / med["a"] * 1e3),
                "gates": {"a < b": med["a"] < med["b"]}, "pass": med["a"] < med["b"] and mis == 0})
    st.close()
    st_l1.close()
    bank.close()
    return res


def host_ms(fns, reps, torch):
    """{key: [the host's milliseconds per call]} of the candidates, enqueue only, in turn within every
    repeat: the queue is drained before each call."""
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            out[k].append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return out


def run_each(name, limit, reps, warmup, variant, seed=2026):
    import numpy as np
    import torch

    from mibminet import lib
    from mibminet.params import ParamSet

    S, n_sets, C, T, N, n_max, ragged = EACH_CASES[name]
    S = min(S, limit)
    n_sets = min(n_sets, S)
    sets = [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(n_sets)]
    bank = lib.Bank(sets)
    set_of = [int(v) for v in np.sort(np.arange(S) * n_sets // S)]
    each = lib.StreamsEach(bank, set_of, HOP, n_max)
    uni = None if ragged else lib.Streams(bank, set_of, HOP, n_max)
    kmax = each.rows(n_max)
    rng = np.random.default_rng(seed)
    lead = T % HOP
    # ticks until every session has its first window: at the mean count n_max / 2, plus the spread
    fill = -(-(T - lead) // (n_max // 2)) + 30 if ragged else -(-(T - lead) // n_max) + 2
    ticks = fill + VERIFY
    total = lead + ticks * n_max
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-128, 128, (S, C, total), dtype=torch.int8, device="cuda", generator=g)
    xh = x.cpu().numpy()
    A = lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    xs = torch.zeros((S, C, n_max), dtype=torch.int8, device="cuda")
    cin = torch.zeros((S,), dtype=torch.int32, device="cuda")
    cout = torch.zeros((S,), dtype=torch.int32, device="cuda")
    ye = torch.zeros((S, kmax, N), dtype=torch.int8, device="cuda")
    yu = torch.zeros((S, n_max // HOP, N), dtype=torch.int8, device="cuda")
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")

    def e():
        rc = A.net_streams_push_each(each.handle, xs.data_ptr(), 1, cin.data_ptr(), n_max, ye.data_ptr(), cout.data_ptr(), None,
                                     nbad.data_ptr(), stream)
        assert rc == 0, rc

    def u():
        rc = A.net_streams_push(uni.handle, xs.data_ptr(), 1, n_max, yu.data_ptr(), nbad.data_ptr(), stream)
        assert rc == 0, rc

    # fill the rings (every session at its own pace in the ragged case), then VERIFY ticks against the reference
    pos = np.zeros(S, np.int64)
    mis = rows_checked = 0
    recipe = None
    for t in range(ticks):
        first_tick = t == 0 and lead > 0
        m = lead if first_tick else n_max
        if ragged and t > 0:
            cnt = rng.integers(0, n_max + 1, size=S).astype(np.int32)
        else:
            cnt = np.full(S, m, np.int32)
        slot = np.zeros((S, C, n_max), np.int8)
        for s in range(S):
            slot[s, :, : cnt[s]] = xh[s, :, pos[s]: pos[s] + cnt[s]]
        xs.copy_(torch.from_numpy(slot))
        cin.copy_(torch.from_numpy(cnt))
        e()
        if uni is not None:
            if first_tick:
                uni.push(x[:, :, :lead].contiguous())
            else:
                u()
        new = pos + cnt
        if t >= fill:
            torch.cuda.synchronize()
            k = np.array([lib.load().net_streams_push_windows(bank.handle, HOP, int(p), int(c)) for p, c in zip(pos, cnt)])
            assert cout.cpu().tolist() == k.tolist()
            if uni is not None:
                assert (k == n_max // HOP).all()
                mis += int((ye[:, : n_max // HOP] != yu).any(dim=2).sum().item())
                rows_checked += int(k.sum())
            else:
                # the recipe: session s from the onset of its first completed window to its last new sample
                W0 = np.where(pos >= T, (pos - T) // HOP + 1, 0)
                lens = np.where(k > 0, new - W0 * HOP, 0)
                starts, Lx, blk_set, onsets, first = lib.bank_windows_lists(bank, lens.tolist(), set_of, HOP)
                assert (np.diff(first) == k).all() and Lx * max(16, C) < 2**31
                xb = np.zeros((C, Lx), np.int8)
                for s in np.flatnonzero(k > 0):
                    xb[:, starts[s]: starts[s] + lens[s]] = xh[s, :, W0[s] * HOP: new[s]]
                wsb = lib.windows_workspace(Lx)
                recipe = (torch.from_numpy(xb).cuda(), Lx, torch.from_numpy(blk_set).cuda(), torch.from_numpy(onsets).cuda(),
                          int(first[-1]), torch.empty((wsb,), dtype=torch.int8, device="cuda"), wsb,
                          torch.empty((int(first[-1]), N), dtype=torch.int8, device="cuda"))
                b_call(A, bank, recipe, nbad, stream)
                torch.cuda.synchronize()
                yb, yeh = recipe[7].cpu().numpy(), ye.cpu().numpy()
                for s in np.flatnonzero(k > 0):
                    mis += int((yeh[s, : k[s]] != yb[first[s]: first[s + 1]]).any(axis=1).sum())
                rows_checked += int(k.sum())
        pos = new
    assert int(nbad.item()) == 0

    # (g): the same enqueue captured once; its replays advance the positions as eager calls do
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rc = A.net_streams_push_each(each.handle, xs.data_ptr(), 1, cin.data_ptr(), n_max, ye.data_ptr(), cout.data_ptr(),
                                         None, nbad.data_ptr(), side.cuda_stream)
            assert rc == 0, rc
    # two rounds, so that a replay never sits between the eager call and its reference: e against the
    # reference, then e against g (its e is reported as device_ms_push_each_beside_graph)
    ref = "u" if uni is not None else "b"
    ref_fn = u if uni is not None else lambda: b_call(A, bank, recipe, nbad, stream)
    ms = time_alternating({"e": e, ref: ref_fn}, reps, warmup)
    ms.update(time_alternating({"e2": e, "g": graph.replay}, reps, warmup))
    med = medians(ms)
    host = host_ms({"e": e, ref: ref_fn}, reps, torch)
    host.update(host_ms({"e2": e, "g": graph.replay}, reps, torch))
    info = bank.info()
    res = {"name": name, "sessions": S, "sets": n_sets, "C": C, "T": T, "N": N, "hop": HOP, "n_max": n_max,
           "counts": "uniform 0 .. n_max" if ragged else "all n_max", "mean_count": round(float(cnt.mean()), 2),
           "rows_per_session": kmax, "windows_last_tick": int(k.sum()), "variant": variant, "exact_division": bool(info[4]),
           "verified_ticks": VERIFY, "rows_verified": rows_checked, "mismatched_rows": mis, "reps": reps, "warmup": warmup,
           "reference": "net_streams_push (uniform group)" if uni is not None else "chunking recipe, net_model_compute_windows_bank",
           "device": torch.cuda.get_device_name(0),
           "device_ms_push_each": round(med["e"], 4), "device_ms_reference": round(med[ref], 4),
           "device_ms_push_each_beside_graph": round(med["e2"], 4), "device_ms_push_each_graph": round(med["g"], 4),
           "host_ms_push_each": round(statistics.median(host["e"]), 4),
           "host_ms_push_each_beside_graph": round(statistics.median(host["e2"]), 4),
           "host_ms_push_each_graph": round(statistics.median(host["g"]), 4),
           "host_ms_reference": round(statistics.median(host[ref]), 4),
           "device_ms_push_each_min_max": min_max(ms["e"]), "device_ms_push_each_graph_min_max": min_max(ms["g"]),
           "device_ms_reference_min_max": min_max(ms[ref]),
           "push_each_over_reference": round(med["e"] / med[ref], 4), "graph_over_eager": round(med["g"] / med["e2"], 4),
           "pass": mis == 0 and rows_checked > 0}
    del graph
    each.close()
    if uni is not None:
        uni.close()
    bank.close()
    return res


def run_f32(name, limit, reps, warmup, variant, seed=2026):
    import numpy as np
    import torch

    from mibminet import lib
    from mibminet.params import ParamSet

    S, n_sets, C, T, N, n, R = F32_CASES[name]
    S = min(S, limit)
    n_sets = min(n_sets, S)
    sets = [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(n_sets)]
    scales = [1.0 + 0.25 * s for s in range(n_sets)]
    bank = lib.Bank(sets, scales)
    montage = R != C
    ch = sorted(int(c) for c in np.random.default_rng(seed).permutation(R)[:C]) if montage else list(range(C))
    wide = lib.Bank([ps.widened(R, ch) for ps in sets], scales) if montage else bank
    set_of = [int(v) for v in np.sort(np.arange(S) * n_sets // S)]
    groups = {key: lib.Streams(wide if key == "new" else bank, set_of, HOP, n) for key in ("new", "a", "b")}
    k = n // HOP
    lead = T % HOP
    fill = -(-(T - lead) // n)
    total = lead + (fill + VERIFY) * n
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((S, total, R), dtype=torch.float32, device="cuda", generator=g)  # frames [S][t][R]
    idx = torch.tensor(ch, dtype=torch.int64, device="cuda")
    xtm = torch.empty((S, n, R), dtype=torch.float32, device="cuda")   # the tick's frames as delivered
    xct = torch.empty((S, C, n), dtype=torch.float32, device="cuda")   # (a)'s and (b)'s transposed chunk
    y = {key: torch.empty((S, k, N), dtype=torch.int8, device="cuda") for key in groups}
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")
    A = lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    def gather():  # what a caller does to the tick's frames at the parent commit
        xct.copy_((xtm.index_select(2, idx) if montage else xtm).transpose(1, 2))

    def new():
        rc = A.net_streams_push_f32_tm(groups["new"].handle, xtm.data_ptr(), n, y["new"].data_ptr(), nbad.data_ptr(), stream)
        assert rc == 0, rc

    def b():
        rc = A.net_streams_push_f32(groups["b"].handle, xct.data_ptr(), n, y["b"].data_ptr(), nbad.data_ptr(), stream)
        assert rc == 0, rc

    def a():
        gather()
        rc = A.net_streams_push_f32(groups["a"].handle, xct.data_ptr(), n, y["a"].data_ptr(), nbad.data_ptr(), stream)
        assert rc == 0, rc

    pos = 0
    for m in [lead] * (lead > 0) + [n] * fill:
        fr = x[:, pos: pos + m].contiguous()
        groups["new"].push_f32(fr, layout="tc")
        ct = fr.index_select(2, idx).transpose(1, 2).contiguous()
        groups["a"].push_f32(ct)
        groups["b"].push_f32(ct)
        pos += m
    assert all(st.windows(n) == k for st in groups.values())
    mis = 0
    for _ in range(VERIFY):
        xtm.copy_(x[:, pos: pos + n])
        new()
        a()  # leaves the transposed chunk in xct for (b)
        b()
        pos += n
        torch.cuda.synchronize()
        mis += int((y["new"] != y["a"]).any(dim=2).sum().item()) + int((y["new"] != y["b"]).any(dim=2).sum().item())
    assert int(nbad.item()) == 0
    ms = time_alternating({"new": new, "a": a, "b": b}, reps, warmup)
    ms["t"] = time_alternating({"t": gather}, reps, warmup)["t"]  # the extra pass alone, for the record
    med = medians(ms)
    info = wide.info()
    res = {"name": name, "sessions": S, "sets": n_sets, "C": C, "source_rows": R, "T": T, "N": N, "hop": HOP, "n": n,
           "windows_per_tick": S * k, "variant": variant, "exact_division": bool(info[4]), "verified_ticks": VERIFY,
           "mismatched_rows": mis, "reps": reps, "warmup": warmup, "device": torch.cuda.get_device_name(0),
           "ms_push_f32_tm": round(med["new"], 4), "ms_transpose_then_push_f32": round(med["a"], 4),
           "ms_push_f32_alone": round(med["b"], 4), "ms_transpose_alone": round(med["t"], 4),
           "ms_push_f32_tm_min_max": min_max(ms["new"]), "ms_transpose_then_push_f32_min_max": min_max(ms["a"]),
           "ms_push_f32_alone_min_max": min_max(ms["b"]),
           "new_over_a": round(med["new"] / med["a"], 4), "new_over_b": round(med["new"] / med["b"], 4),
           "gates": {"new <= a": med["new"] <= med["a"]}, "pass": mis == 0}
    for st in groups.values():
        st.close()
    if montage:
        wide.close()
    bank.close()
    return res


def run_decim(name, limit, reps, warmup, variant, seed=2026):
    import numpy as np
    import torch

    from mibminet import decimate, lib
    from mibminet.params import ParamSet

    S, n_sets, C, T, N, n, settings = DECIM_CASES[name]
    S = min(S, limit)
    n_sets = min(n_sets, S)
    sets = [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(n_sets)]
    scales = [1.0 + 0.25 * s for s in range(n_sets)]
    bank = lib.Bank(sets, scales)
    set_of = [int(v) for v in np.sort(np.arange(S) * n_sets // S)]
    k = n // HOP
    lead = T % HOP
    fill = -(-(T - lead) // n)
    A = lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    configs, mis_all = [], 0
    for q, K in settings:
        taps = decimate.firwin_taps(q, K)
        groups = {key: lib.Streams(bank, set_of, HOP, n) for key in ("new", "a", "b")}
        groups["new"].decimate(q, taps)
        n_raw = q * n
        xraw = torch.zeros((S, n_raw, C), dtype=torch.float32, device="cuda")  # the tick's frames as delivered
        xdec = torch.zeros((S, n, C), dtype=torch.float32, device="cuda")      # (b)'s: decimated beforehand
        tail = torch.zeros((S, K - 1, C), dtype=torch.float32, device="cuda")  # (a)'s kept frames
        weight = torch.from_numpy(np.ascontiguousarray(taps[::-1])).cuda().view(1, 1, K).repeat(C, 1, 1)
        y = {key: torch.empty((S, k, N), dtype=torch.int8, device="cuda") for key in groups}

        def new():
            rc = A.net_streams_push_raw_f32_tm(groups["new"].handle, xraw.data_ptr(), n_raw, y["new"].data_ptr(),
                                               nbad.data_ptr(), stream)
            assert rc == 0, rc

        def a():  # the kept tail, the cat, the strided depthwise convolution, frames again, the push
            with torch.no_grad():
                cat = torch.cat((tail, xraw), dim=1)
                tail.copy_(cat[:, n_raw:])
                dec = torch.nn.functional.conv1d(cat.transpose(1, 2), weight, stride=q, groups=C)  # [S][C][n]
                fr = dec.transpose(1, 2).contiguous()
            rc = A.net_streams_push_f32_tm(groups["a"].handle, fr.data_ptr(), n, y["a"].data_ptr(), nbad.data_ptr(), stream)
            assert rc == 0, rc

        def b():
            rc = A.net_streams_push_f32_tm(groups["b"].handle, xdec.data_ptr(), n, y["b"].data_ptr(), nbad.data_ptr(), stream)
            assert rc == 0, rc

        # zero frames until the first window is one tick away: every position is then T mod hop on the grid
        for m in [lead] * (lead > 0) + [n] * fill:
            groups["new"].push_raw(xraw[:, : q * m].contiguous())
            for key in ("a", "b"):
                groups[key].push_f32(xdec[:, :m].contiguous(), layout="tc")
        assert all(st.info()[4] == lead + fill * n for st in groups.values())
        state, pos = np.zeros((K - 1, S * C), np.float32), q * (lead + fill * n)
        mis = mis_a = 0
        for _ in range(VERIFY):
            xraw.copy_(torch.randn((S, n_raw, C), dtype=torch.float32, device="cuda", generator=g))
            flat = np.ascontiguousarray(xraw.cpu().numpy().transpose(1, 0, 2).reshape(n_raw, S * C))
            dec, state = decimate.fir_decimate(flat, taps, q, state, pos)
            pos += n_raw
            xdec.copy_(torch.from_numpy(np.ascontiguousarray(dec.reshape(n, S, C).transpose(1, 0, 2))))
            new()
            a()
            b()
            torch.cuda.synchronize()
            mis += int((y["new"] != y["b"]).any(dim=2).sum().item())
            mis_a += int((y["new"] != y["a"]).any(dim=2).sum().item())
        assert int(nbad.item()) == 0
        ms = time_alternating({"new": new, "a": a, "b": b}, reps, warmup)
        med = medians(ms)
        configs.append({"q": q, "K": K, "raw_frames_per_tick": n_raw, "mismatched_rows": mis,
                        "rows_of_recipe_that_differ": mis_a, "ms_push_raw_f32_tm": round(med["new"], 4),
                        "ms_tail_cat_conv1d_push_f32_tm": round(med["a"], 4), "ms_push_f32_tm_alone": round(med["b"], 4),
                        "ms_push_raw_f32_tm_min_max": min_max(ms["new"]),
                        "ms_tail_cat_conv1d_push_f32_tm_min_max": min_max(ms["a"]),
                        "ms_push_f32_tm_alone_min_max": min_max(ms["b"]), "new_over_a": round(med["new"] / med["a"], 4),
                        "new_over_b": round(med["new"] / med["b"], 4), "new <= a": med["new"] <= med["a"]})
        mis_all += mis
        for st in groups.values():
            st.close()
    info = bank.info()
    res = {"name": name, "sessions": S, "sets": n_sets, "C": C, "T": T, "N": N, "hop": HOP, "n": n, "windows_per_tick": S * k,
           "variant": variant, "exact_division": bool(info[4]), "verified_ticks": VERIFY, "mismatched_rows": mis_all,
           "reps": reps, "warmup": warmup, "device": torch.cuda.get_device_name(0), "configs": configs,
           "gates": {f"new <= a (q {c['q']}, K {c['K']})": c["new <= a"] for c in configs}, "pass": mis_all == 0}
    bank.close()
    return res


def run_each_raw(name, limit, reps, warmup, variant, seed=2026):
    import numpy as np
    import torch

    from mibminet import decimate, lib
    from mibminet.params import ParamSet

    S, n_sets, C, T, N, n, ragged, settings = EACH_RAW_CASES[name]
    S = min(S, limit)
    n_sets = min(n_sets, S)
    sets = [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(n_sets)]
    scales = [1.0 + 0.25 * s for s in range(n_sets)]
    bank = lib.Bank(sets, scales)
    set_of = [int(v) for v in np.sort(np.arange(S) * n_sets // S)]
    k = n // HOP
    lead = T % HOP
    fill = -(-(T - lead) // n)
    A = lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    configs, mis_all, rows_all = [], 0, 0
    for q, K in settings:
        taps = decimate.firwin_taps(q, K)
        n_raw = q * n  # n_raw_max
        groups = {key: lib.StreamsEach(bank, set_of, HOP, n) for key in ("new", "a", "b")}
        groups["new"].decimate(q, taps)
        uni = None if ragged else lib.Streams(bank, set_of, HOP, n)
        if uni is not None:
            uni.decimate(q, taps)
        kmax = groups["b"].rows(n)
        assert kmax == lib.each_raw_rows(HOP, q, n_raw)
        xraw = torch.zeros((S, n_raw, C), dtype=torch.float32, device="cuda")  # the tick's slots as delivered
        xdec = torch.zeros((S, n, C), dtype=torch.float32, device="cuda")      # (b)'s: decimated beforehand
        cin = torch.full((S,), n_raw, dtype=torch.int32, device="cuda")        # raw counts
        mb = torch.full((S,), n, dtype=torch.int32, device="cuda")             # (b)'s decimated counts
        ma = torch.zeros((S,), dtype=torch.int32, device="cuda")               # (a)'s, computed in the recipe
        tail = torch.zeros((S, K - 1, C), dtype=torch.float32, device="cuda")  # (a)'s kept frames per session
        Pa = torch.zeros((S,), dtype=torch.int64, device="cuda")               # (a)'s raw positions
        weight = torch.from_numpy(np.ascontiguousarray(taps[::-1])).cuda().view(1, 1, K).repeat(C, 1, 1)
        jj = q * torch.arange(n, dtype=torch.int64, device="cuda").view(1, n)
        kk = torch.arange(K - 1, dtype=torch.int64, device="cuda").view(1, K - 1)
        y = {key: torch.zeros((S, kmax, N), dtype=torch.int8, device="cuda") for key in groups}
        cout = {key: torch.zeros((S,), dtype=torch.int32, device="cuda") for key in groups}
        yu = torch.zeros((S, k, N), dtype=torch.int8, device="cuda")

        def new(st=stream):
            rc = A.net_streams_push_each_raw_f32_tm(groups["new"].handle, xraw.data_ptr(), cin.data_ptr(), n_raw,
                                                    y["new"].data_ptr(), cout["new"].data_ptr(), None, nbad.data_ptr(), st)
            assert rc == 0, rc

        def a():  # tails, cat, stride-1 depthwise conv1d, each session's phase gathered, the new tails, the push
            with torch.no_grad():
                cat = torch.cat((tail, xraw), dim=1)  # [S][K - 1 + n_raw][C]
                full = torch.nn.functional.conv1d(cat.transpose(1, 2), weight, groups=C)  # [S][C][n_raw]: output j ends in frame j
                cnt = cin.to(torch.int64)
                off = (-Pa) % q
                ma.copy_((Pa + cnt + (q - 1)) // q - (Pa + (q - 1)) // q)
                idx = (off.view(S, 1) + jj).clamp_(max=n_raw - 1)
                fr = full.gather(2, idx.view(S, 1, n).expand(S, C, n)).transpose(1, 2).contiguous()  # [S][n][C]
                tail.copy_(cat.gather(1, (cnt.view(S, 1) + kk).view(S, K - 1, 1).expand(S, K - 1, C)))
                Pa.add_(cnt)
            rc = A.net_streams_push_each_f32_tm(groups["a"].handle, fr.data_ptr(), ma.data_ptr(), n, y["a"].data_ptr(),
                                                cout["a"].data_ptr(), None, nbad.data_ptr(), stream)
            assert rc == 0, rc

        def b():
            rc = A.net_streams_push_each_f32_tm(groups["b"].handle, xdec.data_ptr(), mb.data_ptr(), n, y["b"].data_ptr(),
                                                cout["b"].data_ptr(), None, nbad.data_ptr(), stream)
            assert rc == 0, rc

        def u():
            rc = A.net_streams_push_raw_f32_tm(uni.handle, xraw.data_ptr(), n_raw, yu.data_ptr(), nbad.data_ptr(), stream)
            assert rc == 0, rc

        # zero frames at equal counts until the first window is one tick away
        for m in [lead] * (lead > 0) + [n] * fill:
            cin.fill_(q * m)
            mb.fill_(m)
            new()
            a()
            b()
            if uni is not None:
                uni.push_raw(xraw[:, : q * m].contiguous())
        torch.cuda.synchronize()
        P = np.full(S, q * (lead + fill * n), np.int64)
        assert groups["new"].raw_positions().tolist() == P.tolist() == Pa.tolist()
        assert groups["new"].positions().tolist() == groups["b"].positions().tolist() == [lead + fill * n] * S
        state = [np.zeros((K - 1, C), np.float32) for _ in range(S)]
        mis = mis_a = rows = 0
        for _ in range(VERIFY):
            cnt = rng.integers(0, n_raw + 1, size=S).astype(np.int32) if ragged else np.full(S, n_raw, np.int32)
            xraw.copy_(torch.randn((S, n_raw, C), dtype=torch.float32, device="cuda", generator=g))
            xh = xraw.cpu().numpy()
            dec, mh = np.zeros((S, n, C), np.float32), np.zeros(S, np.int32)
            for s in range(S):
                d, state[s] = decimate.fir_decimate(np.ascontiguousarray(xh[s, : cnt[s]]), taps, q, state[s], int(P[s]))
                dec[s, : len(d)], mh[s] = d, len(d)
            P += cnt
            xdec.copy_(torch.from_numpy(dec))
            mb.copy_(torch.from_numpy(mh))
            cin.copy_(torch.from_numpy(cnt))
            new()
            a()
            b()
            if uni is not None:
                u()
            torch.cuda.synchronize()
            kc = cout["new"].cpu().numpy()
            assert (kc == cout["b"].cpu().numpy()).all() and (kc == cout["a"].cpu().numpy()).all() and ma.cpu().tolist() == mh.tolist()
            live = torch.arange(kmax, device="cuda").view(1, kmax) < cout["new"].view(S, 1)
            mis += int(((y["new"] != y["b"]).any(dim=2) & live).sum().item())
            mis_a += int(((y["new"] != y["a"]).any(dim=2) & live).sum().item())
            if uni is not None:
                assert (kc == k).all()
                mis += int((y["new"][:, :k] != yu).any(dim=2).sum().item())
            rows += int(kc.sum())
        assert int(nbad.item()) == 0 and groups["new"].raw_positions().tolist() == P.tolist()
        # (g): the same enqueue captured once on one stream; two rounds, as run_each times them
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                new(side.cuda_stream)
        fns = {"new": new, "a": a, "b": b} if ragged else {"new": new, "u": u, "b": b}
        ms = time_alternating(fns, reps, warmup)
        ms.update(time_alternating({"new2": new, "g": graph.replay}, reps, warmup))
        med = medians(ms)
        assert int(nbad.item()) == 0
        c = {"q": q, "K": K, "n_raw_max": n_raw, "mean_count": round(float(cnt.mean()), 2), "rows_verified": rows,
             "mismatched_rows": mis, "rows_of_recipe_that_differ": mis_a,
             "ms_push_each_raw": round(med["new"], 4), "ms_push_each_raw_min_max": min_max(ms["new"]),
             "ms_push_each_f32_tm_decimated_beforehand": round(med["b"], 4), "new_over_b": round(med["new"] / med["b"], 4),
             "ms_push_each_raw_beside_graph": round(med["new2"], 4), "ms_push_each_raw_graph": round(med["g"], 4),
             "graph_over_eager": round(med["g"] / med["new2"], 4)}
        if ragged:
            c.update({"ms_tails_cat_conv1d_gather_push_each_f32_tm": round(med["a"], 4),
                      "ms_tails_cat_conv1d_gather_push_each_f32_tm_min_max": min_max(ms["a"]),
                      "new_over_a": round(med["new"] / med["a"], 4), "new <= a": med["new"] <= med["a"]})
        else:
            c.update({"ms_push_raw_f32_tm_uniform": round(med["u"], 4), "ms_push_raw_f32_tm_uniform_min_max": min_max(ms["u"]),
                      "new_over_u": round(med["new"] / med["u"], 4)})
        configs.append(c)
        mis_all += mis
        rows_all += rows
        del graph
        for st in groups.values():
            st.close()
        if uni is not None:
            uni.close()
    info = bank.info()
    res = {"name": name, "sessions": S, "sets": n_sets, "C": C, "T": T, "N": N, "hop": HOP,
           "counts": "uniform 0 .. n_raw_max" if ragged else "all n_raw_max", "rows_per_session": kmax, "variant": variant,
           "exact_division": bool(info[4]), "verified_ticks": VERIFY, "rows_verified": rows_all, "mismatched_rows": mis_all,
           "reps": reps, "warmup": warmup, "device": torch.cuda.get_device_name(0), "configs": configs,
           "gates": {f"new <= a (q {c['q']}, K {c['K']})": c["new <= a"] for c in configs} if ragged else "none: report only",
           "pass": mis_all == 0 and rows_all > 0}
    bank.close()
    return res


def run_prefilter(name, limit, reps, warmup, variant, seed=2026):
    import numpy as np
    import torch

    from mibminet import decimate, lib
    from mibminet.params import ParamSet

    S, n_sets, C, T, N, n, each, settings = PREFILTER_CASES[name]
    S = min(S, limit)
    n_sets = min(n_sets, S)
    sets = [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(n_sets)]
    scales = [1.0 + 0.25 * s for s in range(n_sets)]
    bank = lib.Bank(sets, scales)
    set_of = [int(v) for v in np.sort(np.arange(S) * n_sets // S)]
    Group = lib.StreamsEach if each else lib.Streams
    A = lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    configs, mis_all, rows_all = [], 0, 0
    for q, K in settings:
        for ragged in ((False, True) if each else (False,)):
            taps, fs = decimate.firwin_taps(q, K), 250.0 * q
            sos = np.concatenate([decimate.butter_sos(4, 0.5, fs, "highpass"), decimate.biquad("notch", 50.0, fs, 30.0)])
            M, n_raw = len(sos), q * n
            groups = {key: Group(bank, set_of, HOP, n) for key in ("new", "p", "a")}
            for st in groups.values():
                st.decimate(q, taps)
            groups["new"].prefilter(sos)
            kmax = lib.each_raw_rows(HOP, q, n_raw) if each else -(-n // HOP)
            xraw = torch.zeros((S, n_raw, C), dtype=torch.float32, device="cuda")  # the tick's frames as delivered
            xfil = torch.zeros((S, n_raw, C), dtype=torch.float32, device="cuda")  # (p)'s and (a)'s: filtered beforehand
            cin = torch.full((S,), n_raw, dtype=torch.int32, device="cuda")
            y = {key: torch.zeros((S, kmax, N), dtype=torch.int8, device="cuda") for key in groups}
            cout = {key: torch.zeros((S,), dtype=torch.int32, device="cuda") for key in groups}
            za = torch.zeros((M, 2, S, C), dtype=torch.float32, device="cuda")     # (a)'s carried state
            coef = [[float(v) for v in row] for row in sos]
            tt = torch.arange(n_raw, dtype=torch.int32, device="cuda")

            def push(key, x, st=stream):
                h = groups[key].handle
                if each:
                    rc = A.net_streams_push_each_raw_f32_tm(h, x.data_ptr(), cin.data_ptr(), n_raw, y[key].data_ptr(),
                                                            cout[key].data_ptr(), None, nbad.data_ptr(), st)
                else:
                    rc = A.net_streams_push_raw_f32_tm(h, x.data_ptr(), n_raw, y[key].data_ptr(), nbad.data_ptr(), st)
                assert rc == 0, rc

            def new(st=stream):
                push("new", xraw, st)

            def p():  # the parent's path: the raw push alone, on the same frames
                push("p", xraw)

            def a():  # the caller's recipe: the recursion frame by frame in torch ops on [S][C], then the raw push
                with torch.no_grad():
                    for t in range(n_raw):
                        v = xraw[:, t]
                        live = (cin > t).view(S, 1) if ragged else None
                        for j, (b0, b1, b2, a1, a2) in enumerate(coef):
                            w = b0 * v + za[j, 0]
                            z1 = (b1 * v - a1 * w) + za[j, 1]
                            z2 = b2 * v - a2 * w
                            if ragged:
                                z1, z2 = torch.where(live, z1, za[j, 0]), torch.where(live, z2, za[j, 1])
                            za[j, 0], za[j, 1] = z1, z2
                            v = w
                        xfil[:, t] = v
                push("a", xfil)

            state = np.zeros((M, 2, S * C), np.float32)
            mis = rows = 0
            # the first windows complete on the way (ragged counts advance a session by n / 2 per tick on average)
            ticks = int((2.5 if ragged else 1.0) * -(-T // n)) + VERIFY
            for _ in range(ticks):
                cnt = rng.integers(0, n_raw + 1, size=S).astype(np.int32) if ragged else np.full(S, n_raw, np.int32)
                xraw.copy_(100.0 + torch.randn((S, n_raw, C), dtype=torch.float32, device="cuda", generator=g))  # a DC offset
                xh, fil = xraw.cpu().numpy(), np.zeros((S, n_raw, C), np.float32)
                st3 = state.reshape(M, 2, S, C)
                for c in np.unique(cnt):  # the sessions of one count side by side, as the R of one call
                    who = np.flatnonzero(cnt == c)
                    if c == 0:
                        continue
                    flat = np.ascontiguousarray(xh[who, :c].transpose(1, 0, 2).reshape(c, -1))
                    yf, z = decimate.sos_filter(flat, sos, np.ascontiguousarray(st3[:, :, who].reshape(M, 2, -1)))
                    fil[who, :c] = yf.reshape(c, len(who), C).transpose(1, 0, 2)
                    st3[:, :, who] = z.reshape(M, 2, len(who), C)
                cin.copy_(torch.from_numpy(cnt))
                xfil.copy_(torch.from_numpy(fil))
                new()
                push("p", xfil)
                torch.cuda.synchronize()
                if each:
                    assert torch.equal(cout["new"], cout["p"])
                    live = torch.arange(kmax, device="cuda").view(1, kmax) < cout["new"].view(S, 1)
                    mis += int(((y["new"] != y["p"]).any(dim=2) & live).sum().item())
                    rows += int(cout["new"].sum().item())
                else:
                    k = lib.load().net_streams_push_windows(bank.handle, HOP, groups["new"].info()[4] - n, n)
                    mis += int((y["new"][:, :k] != y["p"][:, :k]).any(dim=2).sum().item())
                    rows += S * int(k)
            assert int(nbad.item()) == 0, (q, K, ragged, int(nbad.item()), cout["new"].min().item())
            assert rows > 0, (q, K, ragged, groups["new"].info())
            fns = {"new": new, "p": p, "a": a}
            ms = time_alternating(fns, reps, warmup)
            if each:
                graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
                torch.cuda.synchronize()
                with torch.cuda.stream(side):
                    with torch.cuda.graph(graph, stream=side):
                        new(side.cuda_stream)
                ms.update(time_alternating({"new2": new, "g": graph.replay}, reps, warmup))
            med = medians(ms)
            c = {"q": q, "K": K, "M": M, "raw_frames_per_tick": n_raw, "counts": "uniform 0 .. n_raw_max" if ragged else "all n_raw_max",
                 "rows_verified": rows, "mismatched_rows": mis, "ms_raw_push_with_prefilter": round(med["new"], 4),
                 "ms_raw_push_with_prefilter_min_max": min_max(ms["new"]), "ms_raw_push_alone": round(med["p"], 4),
                 "ms_raw_push_alone_min_max": min_max(ms["p"]), "ms_prefilter_cost_per_tick": round(med["new"] - med["p"], 4),
                 "ms_torch_recursion_then_raw_push": round(med["a"], 4), "ms_torch_recursion_then_raw_push_min_max": min_max(ms["a"]),
                 "new_over_a": round(med["new"] / med["a"], 4), "new <= a": med["new"] <= med["a"],
                 "prefilter_info": groups["new"].prefilter_info()}
            if each:
                c.update({"ms_eager_beside_graph": round(med["new2"], 4), "ms_graph_replay": round(med["g"], 4),
                          "graph_over_eager": round(med["g"] / med["new2"], 4)})
                del graph
            configs.append(c)
            mis_all += mis
            rows_all += rows
            for st in groups.values():
                st.close()
    info = bank.info()
    res = {"name": name, "sessions": S, "sets": n_sets, "C": C, "T": T, "N": N, "hop": HOP, "n": n, "variant": variant,
           "prefilter": "butter_sos(4, 0.5 Hz, highpass) + biquad(notch, 50 Hz, Q 30) at fs = 250 q", "exact_division": bool(info[4]),
           "rows_verified": rows_all, "mismatched_rows": mis_all, "reps": reps, "warmup": warmup,
           "device": torch.cuda.get_device_name(0), "configs": configs,
           "gates": {f"new <= a (q {c['q']}, K {c['K']}, {c['counts']})": c["new <= a"] for c in configs},
           "pass": mis_all == 0 and rows_all > 0 and all(c["new <= a"] for c in configs)}
    bank.close()
    return res


def run_at(name, limit, reps, warmup, variant, seed=2026):
    import numpy as np
    import torch

    from mibminet import lib
    from mibminet.params import ParamSet

    S, n_sets, C, T, N, n = AT_CASES[name]
    S = min(S, limit)
    n_sets = min(n_sets, S)
    sets = [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(n_sets)]
    bank = lib.Bank(sets)
    set_of = [int(v) for v in np.sort(np.arange(S) * n_sets // S)]  # grouped: the queries are sorted by session
    st = lib.Streams(bank, set_of, HOP, n)
    cap = st.cap
    fill = -(-cap // n)  # pushes until the ring is full, so that every span is cap - T + 1 onsets
    total = (fill + VERIFY) * n
    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-128, 128, (S, C, total), dtype=torch.int8, device="cuda", generator=g)
    A = lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    xa = x[:, :, :n].contiguous()
    k = n // HOP
    yp = torch.empty((S, max(k, 1), N), dtype=torch.int8, device="cuda")
    yn, yb = (torch.empty((S, N), dtype=torch.int8, device="cuda") for _ in range(2))
    ses = torch.arange(S, dtype=torch.int32, device="cuda")
    sod = torch.tensor(set_of, dtype=torch.int32, device="cuda")
    ons = torch.zeros((S,), dtype=torch.int64, device="cuda")  # (new)'s: on the group's position axis
    onb = torch.zeros((S,), dtype=torch.int64, device="cuda")  # (b)'s: flat element indices of raw
    raw = torch.zeros((S, C, cap), dtype=torch.int8, device="cuda")  # (b): the last cap samples of every session
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")

    def p():
        rc = A.net_streams_push(st.handle, xa.data_ptr(), 1, n, yp.data_ptr(), nbad.data_ptr(), stream)
        assert rc == 0, rc

    def new():
        rc = A.net_streams_windows_at(st.handle, ses.data_ptr(), ons.data_ptr(), S, yn.data_ptr(), nbad.data_ptr(), stream)
        assert rc == 0, rc

    def b():
        rc = A.net_model_compute_epochs_bank(bank.handle, raw.data_ptr(), S * C * cap, cap, None, onb.data_ptr(), sod.data_ptr(),
                                             S, yb.data_ptr(), nbad.data_ptr(), 0, stream)
        assert rc == 0, rc

    def draw(pos):
        """One cue per session inside its span; (b)'s onsets address the same samples in raw."""
        rel = rng.integers(0, cap - T + 1, size=S)
        ons.copy_(torch.from_numpy(rel + (pos - cap)))
        onb.copy_(torch.from_numpy(rel + np.arange(S, dtype=np.int64) * (C * cap)))

    pos = 0
    for _ in range(fill):
        st.push(x[:, :, pos: pos + n].contiguous())
        pos += n
    mis = 0
    for _ in range(VERIFY):
        xa.copy_(x[:, :, pos: pos + n])
        p()
        pos += n
        raw.copy_(x[:, :, pos - cap: pos])
        draw(pos)
        new()
        b()
        torch.cuda.synchronize()
        mis += int((yn != yb).any(dim=1).sum().item())
    assert int(nbad.item()) == 0 and st.at_span() == (pos - cap, pos - T)
    # every timed tick: a push (timed on its own), the cues moved along with the position, then (new) and (b),
    # which take turns going first; raw stays as it is, which flatters (b): a caller rewrites it every tick
    ms = {"p": [], "new": [], "b": []}

    def timed(key, fn, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if keep:
            ms[key].append(e0.elapsed_time(e1))

    for r in range(warmup + reps):
        keep = r >= warmup
        timed("p", p, keep)
        ons.add_(n)
        for key in (("new", "b") if r % 2 else ("b", "new")):
            timed(key, new if key == "new" else b, keep)
    torch.cuda.synchronize()
    assert int(nbad.item()) == 0  # every timed query was valid
    med = medians(ms)
    info = bank.info()
    res = {"name": name, "sessions": S, "sets": n_sets, "C": C, "T": T, "N": N, "hop": HOP, "n": n, "queries_per_tick": S,
           "ring_samples": cap, "onsets": "one per session, uniform in its span of cap - T + 1, sorted by session",
           "variant": variant, "exact_division": bool(info[4]), "verified_ticks": VERIFY, "mismatched_rows": mis,
           "reps": reps, "warmup": warmup, "device": torch.cuda.get_device_name(0),
           "ms_windows_at": round(med["new"], 4), "ms_epochs_bank_on_raw": round(med["b"], 4), "ms_push": round(med["p"], 4),
           "ms_windows_at_min_max": min_max(ms["new"]), "ms_epochs_bank_on_raw_min_max": min_max(ms["b"]),
           "ms_push_min_max": min_max(ms["p"]), "new_over_b": round(med["new"] / med["b"], 4),
           "layer1_samples_b_over_new": "T per window against none (the ring holds them)",
           "not_timed": "(g) a hop-1 group: its grid covers every cue, at hop times the layers 2-5 work per push",
           "gates": {"new <= b": med["new"] <= med["b"]}, "pass": mis == 0}
    st.close()
    bank.close()
    return res


def run_at_feat(name, limit, reps, warmup, variant, seed=2026):
    import numpy as np
    import torch

    from mibminet import lib
    from mibminet.params import ParamSet

    S, n_sets, C, T, N, n = AT_FEAT_CASES[name]
    S = min(S, limit)
    n_sets = min(n_sets, S)
    sets = [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(n_sets)]
    bank = lib.Bank(sets)
    set_of = [int(v) for v in np.sort(np.arange(S) * n_sets // S)]
    st = lib.Streams(bank, set_of, HOP, n)
    cap = st.cap
    fill = -(-cap // n)
    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-128, 128, (S, C, (fill + VERIFY) * n), dtype=torch.int8, device="cuda", generator=g)
    A = lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    xa = x[:, :, :n].contiguous()
    yp = torch.empty((S, max(n // HOP, 1), N), dtype=torch.int8, device="cuda")
    yn, yf = (torch.empty((S, N), dtype=torch.int8, device="cuda") for _ in range(2))
    fb = bank.feature_bytes()
    feat = torch.empty((S, fb), dtype=torch.int8, device="cuda")
    ses = torch.arange(S, dtype=torch.int32, device="cuda")
    ons = torch.zeros((S,), dtype=torch.int64, device="cuda")
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")

    def p():
        rc = A.net_streams_push(st.handle, xa.data_ptr(), 1, n, yp.data_ptr(), nbad.data_ptr(), stream)
        assert rc == 0, rc

    def new():
        rc = A.net_streams_windows_at(st.handle, ses.data_ptr(), ons.data_ptr(), S, yn.data_ptr(), nbad.data_ptr(), stream)
        assert rc == 0, rc

    def with_feat():
        rc = A.net_streams_windows_at_feat(st.handle, ses.data_ptr(), ons.data_ptr(), S, yf.data_ptr(), feat.data_ptr(),
                                           nbad.data_ptr(), stream)
        assert rc == 0, rc

    pos = 0
    for _ in range(fill):
        st.push(x[:, :, pos: pos + n].contiguous())
        pos += n
    mis = 0
    for _ in range(VERIFY):
        xa.copy_(x[:, :, pos: pos + n])
        p()
        pos += n
        ons.copy_(torch.from_numpy(rng.integers(0, cap - T + 1, size=S) + (pos - cap)))
        new()
        with_feat()
        torch.cuda.synchronize()
        mis += int((yn != yf).any(dim=1).sum().item())
    assert int(nbad.item()) == 0
    ms = {"new": [], "new2": [], "feat": []}
    fns = {"new": new, "new2": new, "feat": with_feat}
    order = ["new", "feat", "new2"]
    for r in range(warmup + reps):
        p()
        ons.add_(n)
        for key in order[r % 3:] + order[: r % 3]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns[key]()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[key].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    assert int(nbad.item()) == 0  # every timed query was valid
    med = medians(ms)
    res = {"name": name, "sessions": S, "sets": n_sets, "C": C, "T": T, "N": N, "hop": HOP, "n": n, "queries_per_tick": S,
           "ring_samples": cap, "feature_bytes_per_window": fb, "ring_bytes_read_per_window": 16 * T, "variant": variant,
           "verified_ticks": VERIFY, "mismatched_rows": mis, "reps": reps, "warmup": warmup,
           "device": torch.cuda.get_device_name(0), "ms_windows_at": round(med["new"], 4),
           "ms_windows_at_again": round(med["new2"], 4), "ms_windows_at_feat": round(med["feat"], 4),
           "ms_windows_at_min_max": min_max(ms["new"]), "ms_windows_at_again_min_max": min_max(ms["new2"]),
           "ms_windows_at_feat_min_max": min_max(ms["feat"]), "feat_over_plain": round(med["feat"] / med["new"], 4),
           "plain_again_over_plain": round(med["new2"] / med["new"], 4), "gates": "none: report only", "pass": mis == 0}
    st.close()
    bank.close()
    return res


def b_call(A, bank, recipe, nbad, stream):
    xb, Lx, bsd, ond, W, ws, wsb, yb = recipe
    rc = A.net_model_compute_windows_bank(bank.handle, xb.data_ptr(), 1, Lx, bsd.data_ptr(), ond.data_ptr(), W, yb.data_ptr(),
                                          nbad.data_ptr(), ws.data_ptr(), wsb, 0, stream)
    assert rc == 0, rc



if __name__ == "__main__":
    main(__doc__, {**CASES, **EACH_CASES, **F32_CASES, **DECIM_CASES, **EACH_RAW_CASES, **PREFILTER_CASES, **AT_CASES, **AT_FEAT_CASES}, run_case, "limit", "streams", lambda res: res["mismatched_rows"] + (res["name"] in PREFILTER_CASES and not res["pass"]), reps=1000, warmup=50)
