#!/bin/bash
# One line per kernel instantiation of the families below: its template arguments, VGPRs, SGPR and VGPR
# spills, scratch bytes/lane, LDS bytes and occupancy (waves per SIMD).
#   wg::k_forward (Cfg: C, T, RB, CB, CT, FQ, XR); ep::k_forward_ep (layout, RB, XR, CB); win::k_forward_y1 and
#   win::k_forward_y1_at (RB, XR, CB); gen::k_forward (layout, staged, RB, XR, CB) and gen::k_layer (RB, XR, CB);
#   bank::k_forward_ep_bank and _feat (layout, RB, XR, CB), bank::k_forward_y1_bank (RB, XR, CB);
#   stream::k_forward_ring and _each (RB, XR, CB), stream::k_forward_ring_at and _feat (RB, XR, CB, EACH),
#   stream::k_layer1_ring and _each (layout, XR, CB).
# usage: tools/resource.sh [repo root | file]  (default: this checkout; a file: the compiler's
#        -Rpass-analysis=kernel-resource-usage remarks of another build, read as they are)
SRC="${1:-$(dirname "$0")/..}"
if [ -f "$SRC" ]; then cat "$SRC"; else make -s -C "$SRC/mi-bminet_amd" resource 2>&1; fi | python3 -c '
import re, sys
A3 = r"ILb(\d)ELb(\d)ELb(\d)E"
A4 = r"ILb(\d)ELb(\d)ELb(\d)ELb(\d)E"
L3 = r"ILi(\d)ELb(\d)ELb(\d)E"
L4 = r"ILi(\d)ELb(\d)ELb(\d)ELb(\d)E"
FAMILIES = [  # (mangled prefix and template list, label)
    (r"_ZN3mib2wg9k_forwardINS0_3CfgILi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)", "C=%s T=%s RB=%s CB=%s CT=%s FQ=%s XR=%s"),
    (r"_ZN3mib2ep12k_forward_ep" + L4, "ep L=%s RB=%s XR=%s CB=%s"),  # layout 1 = int8, 2 = float32
    (r"_ZN3mib3win12k_forward_y1" + A3, "win RB=%s XR=%s CB=%s"),
    (r"_ZN3mib3win15k_forward_y1_at" + A3, "win_at RB=%s XR=%s CB=%s"),
    (r"_ZN3mib3gen9k_forwardILi(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", "gen L=%s ST=%s RB=%s XR=%s CB=%s"),
    (r"_ZN3mib3gen7k_layer" + A3, "gen_layer RB=%s XR=%s CB=%s"),
    (r"_ZN3mib4bank17k_forward_ep_bank" + L4, "ep_bank L=%s RB=%s XR=%s CB=%s"),
    (r"_ZN3mib4bank22k_forward_ep_bank_feat" + L4, "ep_bank_feat L=%s RB=%s XR=%s CB=%s"),
    (r"_ZN3mib4bank17k_forward_y1_bank" + A3, "win_bank RB=%s XR=%s CB=%s"),
    (r"_ZN3mib6stream14k_forward_ring" + A3, "ring RB=%s XR=%s CB=%s"),
    (r"_ZN3mib6stream19k_forward_ring_each" + A3, "ring_each RB=%s XR=%s CB=%s"),
    (r"_ZN3mib6stream17k_forward_ring_at" + A4, "ring_at RB=%s XR=%s CB=%s EACH=%s"),
    (r"_ZN3mib6stream22k_forward_ring_at_feat" + A4, "ring_at_feat RB=%s XR=%s CB=%s EACH=%s"),
    (r"_ZN3mib6stream13k_layer1_ring" + L3, "l1_ring L=%s XR=%s CB=%s"),
    (r"_ZN3mib6stream18k_layer1_ring_each" + L3, "l1_ring_each L=%s XR=%s CB=%s"),
]
KEYS = [("VGPRs:", "vgpr"), ("SGPRs Spill:", "sgpr_spill"), ("VGPRs Spill:", "vgpr_spill"), ("ScratchSize [bytes/lane]:", "scratch"),
        ("LDS Size [bytes/block]:", "lds"), ("Occupancy [waves/SIMD]:", "occ")]
cur = None
for line in sys.stdin:
    if "Function Name:" in line:
        cur = None
        for pat, label in FAMILIES:
            m = re.search("Function Name: " + pat, line)
            if m:
                cur, vals = label % m.groups(), {}
                break
        continue
    if cur is None:
        continue
    for k, short in KEYS:
        m = re.search(re.escape(k) + r" (\d+)", line)
        if m:
            vals[short] = m.group(1)
    if len(vals) == len(KEYS):
        print(cur, "".join("  %s %s" % (short, vals[short]) for _, short in KEYS)); cur = None
'
