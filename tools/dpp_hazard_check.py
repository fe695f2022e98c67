"""The DPP wait states of the hand-written row broadcasts (row_bcast_f64, fmac_row_bcast, ... of csrc/dsge_device.hpp), read off a
hipcc -S listing: python tools/dpp_hazard_check.py file.s [symbol substring, default kalman_mf_kernel]

A VALU write of a VGPR needs two wait states before a DPP instruction reads that VGPR as its DPP operand (src0); the compiler's
hazard handling does not look into assembly text.  For every 64-bit DPP instruction (v_mov_b64_dpp, v_fmac_f64_dpp) of every kernel
whose symbol contains the substring, the instructions in front of it are walked back IN LISTING ORDER (over labels: a fall-through
predecessor is the nearest one; a branch only adds distance) to the nearest v_* instruction whose destination overlaps the DPP
operand (an s_nop N counts N + 1 wait states); fewer than two wait states between them is a violation.  A lane swap
(v_permlane16_swap_b32, v_permlane32_swap_b32) writes BOTH its operands and counts as a writer of either.  Also flags a v_cmpx within five wait states in
front of a DPP instruction (EXEC written by the VALU).  Prints per kernel: VGPRs, scratch bytes, the counts of the DPP forms, of
v_readlane_b32 and of the lane swaps, the smallest distance found (wait states between a VALU write of a DPP operand and its read, looking LOOK wait states
back), the violations.  Exit status 1 if there is any.
"""
import re
import sys

LOOK = 12  # wait states walked back for the nearest writer of a DPP operand
SWAPS = ("v_permlane16_swap_b32", "v_permlane32_swap_b32")


def regs(tok):
    tok = tok.strip().lstrip("-|").rstrip(",|")
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def written(ins):
    """VGPRs a v_* instruction writes: its first operand; a lane swap writes both."""
    ops = ins.split(None, 1)[1].split(",")
    out = regs(ops[0])
    if ins.split()[0].startswith(SWAPS) and len(ops) > 1:
        out |= regs(ops[1].split()[0])
    return out


def main():
    text = open(sys.argv[1]).read()
    want = sys.argv[2] if len(sys.argv) > 2 else "kalman_mf_kernel"
    bad = 0
    for m in re.finditer(r"^(_Z\w+):\s*; @", text, re.M):
        sym = m.group(1)
        if want not in sym:
            continue
        end = text.index(".Lfunc_end", m.end())
        tail = text[end:end + 6000]
        ins = []
        for line in text[m.end():end].split("\n"):
            t = line.split(";")[0].strip()
            if t and not t.startswith(".") and not t.endswith(":"):
                ins.append(t)
        n_dpp64 = n_rl = n_swap = 0
        dmin, viol = 99, []
        for k, t in enumerate(ins):
            op = t.split()[0]
            n_rl += op == "v_readlane_b32"
            n_swap += op.startswith(SWAPS)
            if op not in ("v_mov_b64_dpp", "v_fmac_f64_dpp"):
                continue
            n_dpp64 += 1
            src = regs(t.split(None, 1)[1].split(",")[1].split()[0])
            states, b = 0, k - 1
            while b >= 0 and states < LOOK:
                pt = ins[b]
                pop = pt.split()[0]
                if pop.startswith("v_cmpx") and states < 5:
                    viol.append((k, "v_cmpx %d wait states ahead of: %s" % (states, t)))
                if pop.startswith("v_") and written(pt) & src:
                    dmin = min(dmin, states)
                    if states < 2:
                        viol.append((k, "%s  <- %d wait states after: %s" % (t, states, pt)))
                    break
                states += (int(pt.split()[1]) + 1) if pop == "s_nop" else 1
                b -= 1
        vg = re.search(r"; NumVgprs: (\d+)", tail)
        sc = re.search(r"; ScratchSize: (\d+)", tail)
        print(f"{sym}\n  VGPRs {vg.group(1) if vg else '?'}, scratch {sc.group(1) if sc else '?'} B, 64-bit DPP instructions {n_dpp64}, "
              f"v_readlane_b32 {n_rl}, lane swaps {n_swap}, nearest VALU write of a DPP operand {dmin if dmin < 99 else 'more than %d' % LOOK} wait states back, "
              f"violations {len(viol)}")
        for _, v in viol:
            print("   ", v)
        bad += len(viol)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
