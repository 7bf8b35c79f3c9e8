#!/bin/bash
# One line per k_forward instantiation: Cfg template args (C, T, RB, CB, CT, FQ, XR), VGPRs, scratch bytes/lane, LDS bytes.
# The same for each ep::k_forward_ep instantiation (layout, RB, XR, CB) and each win::k_forward_y1 and
# win::k_forward_y1_at (RB, XR, CB), and each bank::k_forward_ep_bank (layout, RB, XR, CB) and
# bank::k_forward_y1_bank (RB, XR, CB).
# usage: tools/resource.sh [repo root]  (default: this checkout)
cd "${1:-$(dirname "$0")/..}/mi-bminet_amd"
make -s resource 2>&1 | python3 -c '
import re, sys
cur = None
for line in sys.stdin:
    m = re.search(r"Function Name: _ZN3mib2wg9k_forwardINS0_3CfgILi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)", line)
    if m:
        cur = "C=%s T=%s RB=%s CB=%s CT=%s FQ=%s XR=%s" % m.groups(); vals = {}
        continue
    m = re.search(r"Function Name: _ZN3mib2ep12k_forward_epILi(\d)ELb(\d)ELb(\d)ELb(\d)E", line)
    if m:  # the epoch kernels (forward_ep.hpp): layout 1 = int8, 2 = float32
        cur = "ep L=%s RB=%s XR=%s CB=%s" % m.groups(); vals = {}
        continue
    m = re.search(r"Function Name: _ZN3mib3win1[25]k_forward_y1(_at)?ILb(\d)ELb(\d)ELb(\d)E", line)
    if m:  # the window kernels (forward_win.hpp): regular onsets, and onsets from a device list
        cur = "win%s RB=%s XR=%s CB=%s" % (m.group(1) or "", *m.groups()[1:]); vals = {}
        continue
    m = re.search(r"Function Name: _ZN3mib4bank17k_forward_ep_bankILi(\d)ELb(\d)ELb(\d)ELb(\d)E", line)
    if m:  # the epochs of a bank (forward_bank.hpp)
        cur = "ep_bank L=%s RB=%s XR=%s CB=%s" % m.groups(); vals = {}
        continue
    m = re.search(r"Function Name: _ZN3mib4bank17k_forward_y1_bankILb(\d)ELb(\d)ELb(\d)E", line)
    if m:  # the windows of a bank
        cur = "win_bank RB=%s XR=%s CB=%s" % m.groups(); vals = {}
        continue
    if cur is None:
        continue
    for k in ("VGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"):
        m = re.search(re.escape(k) + r": (\d+)", line)
        if m:
            vals[k.split()[0]] = m.group(1)
    if len(vals) == 3:
        print(cur, " vgpr", vals["VGPRs"], " scratch", vals["ScratchSize"], " lds", vals["LDS"]); cur = None
'
