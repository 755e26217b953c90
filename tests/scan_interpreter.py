"""A one-lane interpreter for the scans tools/gen_row_bound_packed_asm.py writes (the packed scan and the two
ring scans), for the tests that check them without a GPU.

It knows the handful of instructions the generator emits and nothing else (an unknown one raises).  LDS reads are an
in-order queue: ds_read_b32 takes its address when it is issued and delivers its value only when an s_waitcnt
lgkmcnt(n) drains the queue down to n entries -- the latest moment the hardware allows, so a value that the code uses
earlier than its wait covers cannot be right by luck.  While a read is outstanding its destination register is
`pending`: any instruction that reads it, and any that overwrites it (a new issue into the same register included),
raises Hazard.  A scan must also leave no read outstanding when it falls out of its last label."""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GENERATOR = ROOT / "tools" / "gen_row_bound_packed_asm.py"
M32 = 0xffffffff


class Hazard(AssertionError):
    pass


def generated(*args):
    """The generator's output for `args`, as text."""
    return subprocess.run([sys.executable, str(GENERATOR), *args], capture_output=True, text=True, check=True).stdout


def scan_lines(text):
    """The instructions and labels of the *_SCAN_ASM macro in a generated .inc."""
    lines, on = [], False
    for ln in text.splitlines():
        if re.match(r"#define \w+_SCAN_ASM \\$", ln):
            on = True
        elif on:
            mt = re.match(r'\s*"(.*)\\n\\t"( \\)?$', ln)
            if not mt:
                break
            lines.append(mt.group(1))
    assert lines, "no *_SCAN_ASM macro"
    return lines


def s32(x):
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


class Program:
    def __init__(self, lines):
        self.ops, self.labels = [], {}
        for ln in lines:
            if ln.endswith(":"):
                self.labels[ln[:-1]] = len(self.ops)
                continue
            name, _, rest = ln.partition(" ")
            self.ops.append((name, [x.strip() for x in rest.split(",")] if rest else []))

    def run(self, vregs, sregs, table, max_steps=100000):
        """vregs: register name (as written in the asm: 'v76', '%[C]') -> u32; sregs: name -> int; table: callable (byte
        address, name of the offset operand: 'TOFF', the table) -> u32 word.  Returns the
        register file after the scan; raises Hazard on a wait that does not cover a use."""
        v, queue, pending = dict(vregs), [], set()
        scc, vcc = 0, 0

        def rd(x):
            if x in pending:
                raise Hazard(f"{x} is read while its ds_read is outstanding")
            if x in v:
                return v[x]
            if x in sregs:
                return sregs[x] & M32
            return int(x, 0) & M32

        def wr(x, val):
            if x in pending:
                raise Hazard(f"{x} is overwritten while its ds_read is outstanding")
            v[x] = val & M32

        pc = 0
        for _ in range(max_steps):
            if pc == len(self.ops):
                if queue:
                    raise Hazard(f"{len(queue)} reads outstanding at the end of the scan")
                return v
            name, a = self.ops[pc]
            pc += 1
            if name == "v_mov_b32":
                wr(a[0], rd(a[1]))
            elif name == "v_sub_u32":
                wr(a[0], rd(a[1]) - rd(a[2]))
            elif name == "v_lshrrev_b32":
                wr(a[0], rd(a[2]) >> (rd(a[1]) & 31))
            elif name == "ds_read_b32":
                dst, src = a[0], a[1]
                mt = re.fullmatch(r"(\S+) offset:%c\[(\w+)\]", src)
                assert mt, src
                addr, area = rd(mt.group(1)), mt.group(2)
                if dst in pending:
                    raise Hazard(f"{dst} is the target of a second ds_read while the first is outstanding")
                queue.append((dst, table(addr, area) & M32))
                pending.add(dst)
            elif name == "v_mad_u32_u16":
                wr(a[0], (rd(a[1]) & 0xffff) * (rd(a[2]) & 0xffff) + rd(a[3]))
            elif name == "v_max3_i32":
                wr(a[0], max(s32(rd(a[1])), s32(rd(a[2])), s32(rd(a[3]))))
            elif name == "v_max_i32":
                wr(a[0], max(s32(rd(a[1])), s32(rd(a[2]))))
            elif name == "v_cndmask_b32_e32":
                assert a[3] == "vcc"
                wr(a[0], rd(a[2]) if vcc else rd(a[1]))
            elif name == "s_cmp_gt_i32":
                scc = int(s32(rd(a[0])) > s32(rd(a[1])))
            elif name == "s_cmp_lt_i32":
                scc = int(s32(rd(a[0])) < s32(rd(a[1])))
            elif name == "s_cselect_b64":
                assert a[0] == "vcc"
                vcc = rd(a[1]) if scc else rd(a[2])
            elif name == "s_cbranch_scc0":
                if not scc:
                    pc = self.labels[a[0]]
            elif name == "s_branch":
                pc = self.labels[a[0]]
            elif name == "s_waitcnt":
                mt = re.fullmatch(r"lgkmcnt\((\d+)\)", a[0])
                assert mt and len(a) == 1, a
                while len(queue) > int(mt.group(1)):
                    dst, val = queue.pop(0)
                    pending.discard(dst)
                    v[dst] = val
            else:
                raise AssertionError(f"the interpreter does not know {name}")
        raise AssertionError("the scan does not end")
