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

  python tools/bench_streams.py [--cases mmmi_64,bci_1024,bci_1024_shuffled] [--limit S] [--reps 1000]
                                [--warmup 50] [--variant canonical|plain_bn] [--out-dir profiles]
"""
from bench_common import main, medians, min_max, time_alternating

HOP = 8
VERIFY = 6  # ticks run through both candidates on the same samples
CASES = {  # name: (sessions, sets, C, T, N, n, sets shuffled over the sessions)
    "mmmi_64": (64, 64, 64, 480, 2, 8, False),
    "bci_1024": (1024, 16, 22, 1125, 4, 16, False),
    "bci_1024_shuffled": (1024, 16, 22, 1125, 4, 16, True),
}


def run_case(name, limit, reps, warmup, variant, seed=2026):
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


if __name__ == "__main__":
    main(__doc__, CASES, run_case, "limit", "streams", lambda res: res["mismatched_rows"], reps=1000, warmup=50)
