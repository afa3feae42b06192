"""tools/asm_counts.py on a hand-written assembly listing: instruction classes, the resource lines, template names, --against."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_counts  # noqa: E402

LISTING = """\t.text
_ZN12_GLOBAL__N_16kernelILi4ELb1ELb0EEEvPf: ; @kernel
; %bb.0:
\ts_load_dword s0, s[0:1], 0x0
\ts_waitcnt lgkmcnt(0)
\tv_mov_b32_e32 v0, 0
.LBB0_1: ; in Loop
\tds_read_b128 v[4:7], v1
\tv_mfma_f32_16x16x32_bf16 v[8:11], v[4:7], v[4:7], v[8:11]
\tglobal_store_dwordx4 v[2:3], v[8:11], off
\ts_endpgm
.Lfunc_end0:
; NumVgprs: {vgpr}
; NumAgprs: 0
; ScratchSize: 0
; Occupancy: 8
plain_kernel:
\tv_add_u32_e32 v0, v0, v0
\ts_endpgm
.Lfunc_end1:
; NumVgprs: 1
; Occupancy: 8
"""


def test_counts_names_and_comparison(tmp_path):
    new, old = tmp_path / "new.s", tmp_path / "old.s"
    new.write_text(LISTING.format(vgpr=12))
    old.write_text(LISTING.format(vgpr=16))
    rows = asm_counts.parse(str(new))
    assert [n for n, _ in rows] == ["_ZN12_GLOBAL__N_16kernelILi4ELb1ELb0EEEvPf", "plain_kernel"]
    k = rows[0][1]
    assert (k["VALU"], k["SALU"], k["LDS"], k["VMEM"], k["MFMA"], k["NumVgprs"], k["Occupancy"]) == (1, 3, 1, 1, 1, 12, 8)
    assert rows[1][1]["VALU"] == 1 and rows[1][1]["SALU"] == 1
    assert asm_counts.short("_ZN12_GLOBAL__N_16kernelILi4ELb1ELb0EEEvPf") == "kernel<4, true, false>"
    assert asm_counts.short("void (anonymous namespace)::other<2>(float*)") == "other<2>"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asm_counts.py"), str(new), "--against", str(old), "kernel<"],
                         capture_output=True, text=True, check=True).stdout.split("\n")
    assert len([ln for ln in out if ln.strip()]) == 2 and "kernel<4, true, false>" in out[1] and "16 12" in out[1]
