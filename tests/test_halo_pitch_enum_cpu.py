"""tools/halo_pitch_enum.py --mfma16: the bank-conflict enumeration of the halo kernel's LDS reads on the operand map of
v_mfma_f32_16x16x32 (96-byte rows), against what the header of csrc/conv3d_halo.hpp states for the pitches it ships."""
import importlib.util
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("halo_pitch_enum", os.path.join(ROOT, "tools", "halo_pitch_enum.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header():
    with open(os.path.join(ROOT, "sgcdet_amd", "csrc", "conv3d_halo.hpp")) as f:
        return f.read()


def test_the_shipped_pitches_have_the_conflict_counts_the_header_states():
    enum, src = _tool(), _header()
    m = re.search(r"halo_pitch\(int BZ, int MF = 32\) \{ return BZ == 8 \? (\d+) : BZ == 10 \? \(MF == 16 \? (\d+) : (\d+)\)", src)
    assert m, "halo_pitch() no longer has the form this test reads"
    p8, p10_16, p10_32 = (int(v) for v in m.groups())
    assert enum.LDKH16 * 2 == 96 and "return MF == 16 ? BK + 16 : LDKH" in src           # 96-byte rows (BK = 32 bf16 + 16)
    # the weight tile and the 4 x 8 x 8 brick read conflict-free
    assert enum.count16_weights()[:2] == (0, 0)
    assert enum.count16(4, 8, 8, p8, True)[:2] == (0, 0)
    # 2 x 10 x 10: the header lists the conflicting groups of 32 at the pitches 12..16 and ships the fewest
    stated = re.search(r"BZ = 10 keeps ([\d, ]+) conflicting groups of 32 at the pitches 12\.\.16", src)
    assert stated, "the header no longer states the 2 x 10 x 10 counts"
    counts = [enum.count16(2, 10, 10, pitch, True)[0] for pitch in range(12, 17)]
    assert counts == [int(v) for v in stated.group(1).split(",")]
    assert counts[p10_16 - 12] == min(counts) and enum.count16(2, 10, 10, p10_16, True)[2] == 32
    # the LDS plans stay within 160 KB
    assert enum.count16(4, 8, 8, p8, True)[3] <= 160 * 1024 and enum.count16(2, 10, 10, p10_16, True)[3] <= 160 * 1024
    # the 32x32x16 map is what it was: 0 for 4 x 8 x 8, 7 of 16 for 2 x 10 x 10 at its pitch
    assert enum.count(4, 8, 8, p8, True)[0] == 0 and enum.count(2, 10, 10, p10_32, True)[:3] == (7, 7, 16)


def test_an_odd_row_pitch_cannot_be_conflict_free_on_this_map():
    """The reason for the 96-byte rows: on 80-byte rows every group of the weight tile keeps a conflict."""
    enum = _tool()
    g, _, n = enum.count16_weights(row_chunks=5)
    assert g == n == 16


def test_the_command_line_reports_both_bricks_and_the_weight_tile(capsys, monkeypatch):
    enum = _tool()
    monkeypatch.setattr(sys, "argv", ["halo_pitch_enum.py", "--mfma16"])
    enum.main()
    out = capsys.readouterr().out
    assert "16x16x32 operand map" in out and re.search(r"^\s+14\s+6 of  32", out, re.M)
    assert "weight tile, 96-byte rows: 0 of 16 groups conflict" in out
    monkeypatch.setattr(sys, "argv", ["halo_pitch_enum.py", "4", "8", "8", "--td", "--mfma16"])
    enum.main()
    assert re.search(r"^\s+12\s+0 of  32", capsys.readouterr().out, re.M)
