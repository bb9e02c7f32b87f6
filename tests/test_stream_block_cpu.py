"""CPU: the whole-block kernels and the WS_STREAM_BLOCK_KERNEL flag through the real libraries -- every refusal of
`ws_tcn_block_stream_fwd` / `ws_tcn_block_stream_rows_fwd` with nothing launched, the header's macros, and on a dry-run engine
the launch figure per group with and without the flag (stream and pool), the unchanged state size, the flag's refusals and
`separate_main --stream_ms 10 --stream_block [--stream_pool 3] --dry_run`.  Without the feature every test fails (no symbol,
no macro, no keyword, no option)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_stream_pool_cpu import EMB, G, KW, _export, _write_wav, needs_no_gpu
from wesep_amd import _lib as L
from wesep_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = KW["R"] * KW["X"]
HIP_H = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
ENGINE_H = open(os.path.join(ROOT, "include", "wesep_engine.h")).read()


def test_symbols_are_declared_bound_and_exported():
    lib = L.lib()
    for name, nargs in (("ws_tcn_block_stream_fwd", 27), ("ws_tcn_block_stream_rows_fwd", 30)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", HIP_H, flags=re.M)
        assert m, f"{name} is not declared in wesep_hip.h"
        res, args = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")) == nargs, name
        assert name in L.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    from wesep_amd import dev
    assert callable(dev.tcn_block_stream_fwd) and callable(dev.tcn_block_stream_rows_fwd)
    assert lib.ws_abi_version() == 20 == L.ABI_VERSION and re.search(r"^#define WS_ABI_VERSION 20\b", HIP_H, flags=re.M)
    assert re.search(r"^#define WS_TCN_MID_MAXH 4096\b", HIP_H, flags=re.M)
    assert re.search(r"^#define WS_TCN_BLOCK_MAXH (\d+)", HIP_H, flags=re.M).group(1) == "768"
    assert re.search(r"^#define WS_TCN_BLOCK_MAXB (\d+)", HIP_H, flags=re.M).group(1) == "512"


def test_engine_header_macros_old_and_new():
    flat = lambda s: s.replace(" ", "")
    for line in ("#define WS_STREAM_BLOCK_KERNEL 1", "#define WS_STREAM_BLOCK_GROUP_LAUNCHES(R, X) ((R) * (X) + 10)",
                 "#define WS_POOL_BLOCK_GROUP_LAUNCHES(R, X) ((R) * (X) + 9)", "#define WS_STREAM_GROUP_LAUNCHES(R, X) (3 * (R) * (X) + 10)",
                 "#define WS_POOL_GROUP_LAUNCHES(R, X) (3 * (R) * (X) + 9)", "#define WS_ENGINE_ABI_VERSION 2"):
        assert flat(line) in flat(ENGINE_H), line
    assert E.lib().ws_engine_abi_version() == 2 == E.ENGINE_ABI_VERSION
    assert E.STREAM_BLOCK_KERNEL == 1 and E.stream_block_group_launches(4, 8) == 42 and E.pool_block_group_launches(4, 8) == 41
    assert E.pool_group_launches(4, 8) == 105


def _kernel_args():
    bufs = [(ctypes.c_float * 16384)() for _ in range(19)]
    names = ("x", "rb", "W1", "b1", "a1", "g1", "be1", "wd", "bd", "a2", "g2", "be2", "W2", "b2", "ring", "out", "slot", "t0", "tc")
    return dict(zip(names, (ctypes.cast(v, ctypes.c_void_p) for v in bufs)))


def test_kernels_refuse_bad_arguments_before_any_launch():
    lib, p = L.lib(), _kernel_args()
    err = lambda: lib.ws_last_error().decode()
    eps = ctypes.c_float(1e-5)

    def solo(R=2, Tc=5, B=8, H=8, P=3, dil=4, t0=0, cap=13, ldw1=8, **kw):
        a = {**p, "rb": None, **kw}
        return lib.ws_tcn_block_stream_fwd(a["x"], a["rb"], a["W1"], ldw1, a["b1"], a["a1"], a["g1"], a["be1"], a["wd"], a["bd"], a["a2"],
                                           a["g2"], a["be2"], a["W2"], a["b2"], R, Tc, B, H, P, dil, eps, t0, cap, a["ring"], a["out"], None)

    def rows(A=2, Tc=5, B=8, H=8, P=3, dil=4, nslots=3, cap=13, ldw1=8, **kw):
        a = {**p, "rb": None, **kw}
        return lib.ws_tcn_block_stream_rows_fwd(a["x"], a["rb"], a["W1"], ldw1, a["b1"], a["a1"], a["g1"], a["be1"], a["wd"], a["bd"],
                                                a["a2"], a["g2"], a["be2"], a["W2"], a["b2"], A, Tc, B, H, P, dil, eps, nslots, a["slot"],
                                                a["t0"], a["tc"], cap, a["ring"], a["out"], None)

    for call, who in ((solo, "ws_tcn_block_stream_fwd"), (rows, "ws_tcn_block_stream_rows_fwd")):
        for name in ("x", "W1", "a1", "g1", "be1", "wd", "bd", "a2", "g2", "be2", "W2", "b2", "ring", "out"):
            assert call(**{name: None}) == -1 and f"{who}: null pointer" in err(), (who, name)
        assert call(rb=p["rb"]) == -1 and "exactly one of rb (the row bias) and b1" in err()          # both given
        assert call(b1=None) == -1 and "exactly one of rb (the row bias) and b1" in err()             # neither
        assert call(B=6, ldw1=8) == -1 and "B=6, H=8 and ldw1=8 must be multiples of 4" in err()
        assert call(H=6) == -1 and "must be multiples of 4" in err()
        assert call(ldw1=10) == -1 and "ldw1=10 must be multiples of 4" in err()
        assert call(ldw1=4) == -1 and "ldw1=4 is below B=8" in err()
        assert call(H=772) == -1 and "H=772 above 768" in err()
        assert call(B=516, ldw1=516) == -1 and "B=516 above 512" in err()
        assert call(P=4, cap=17) == -1 and "P=4 (odd P <= 7)" in err()
        assert call(P=9, cap=37) == -1 and "P=9 (odd P <= 7)" in err()
        assert call(dil=0) == -1 and "bad geometry" in err()
        assert call(cap=12) == -1 and "cap=12 is below (P - 1) * dil + Tc = 13" in err()
        assert call(out=p["x"]) == -1 and "out overlaps x" in err()
    assert solo(t0=-1) == -1 and "t0=-1 is negative" in err()
    assert rows(A=0) == -1 and "bad tables (A=0 rows, nslots=3)" in err()
    assert rows(nslots=0) == -1 and "bad tables (A=2 rows, nslots=0)" in err()
    for name in ("slot", "t0", "tc"):
        assert rows(**{name: None}) == -1 and "a NULL table" in err(), name


def _stream_launches(eng, block_kernel):
    """One push that completes 9 frames with max_chunk_frames 4: three groups."""
    st = eng.stream(2, np.zeros((2, 256), np.float32), E.ENROLL_EMBEDDING, max_chunk_frames=G, block_kernel=block_kernel)
    state = eng.info("stream_state_bytes")
    out = st.push(np.zeros((2, 160 + 8 * 10), np.float32))
    n = eng.info("n_launches")
    assert out.shape == (2, 90)
    st.flush()
    st.close()
    return n, state


def _pool_launches(eng, block_kernel):
    pool = eng.stream_pool(3, max_chunk_frames=G, block_kernel=block_kernel)
    state = eng.info("stream_state_bytes")
    a, b = pool.attach(EMB, E.ENROLL_EMBEDDING), pool.attach(EMB, E.ENROLL_EMBEDDING)
    out = pool.push({a: np.zeros(160 + 8 * 10, np.float32), b: np.zeros(165, np.float32)})      # 9 frames and 1: three groups
    n = eng.info("n_launches")
    assert out[a].shape == (90,) and out[b].shape == (10,)
    pool.flush(a)
    assert eng.info("n_launches") % ((RX + 9) if block_kernel else (3 * RX + 9)) == 0
    pool.close()
    return n, state


@needs_no_gpu
def test_launch_figures_with_and_without_the_flag_and_equal_state(tmp_path):
    eng = E.Engine(_export(tmp_path), dry_run=True)
    n_old, state_old = _stream_launches(eng, False)
    n_new, state_new = _stream_launches(eng, True)
    assert n_old == 3 * (3 * RX + 10) and n_new == 3 * (RX + 10) == 3 * E.stream_block_group_launches(KW["R"], KW["X"])
    assert state_old == state_new > 0
    p_old, pstate_old = _pool_launches(eng, False)
    p_new, pstate_new = _pool_launches(eng, True)
    assert p_old == 3 * (3 * RX + 9) and p_new == 3 * (RX + 9) == 3 * E.pool_block_group_launches(KW["R"], KW["X"])
    assert pstate_old == pstate_new > 0
    eng.close()


@needs_no_gpu
def test_flag_refusals(tmp_path):
    eng = E.Engine(_export(tmp_path), dry_run=True)
    h = ctypes.c_void_p()
    emb = np.zeros((2, 256), np.float32)
    assert E.lib().ws_engine_stream_open_ex(eng._h, 2, emb.ctypes.data, E.ENROLL_EMBEDDING, 0, G, 6, ctypes.byref(h)) == -1
    assert "ws_engine_stream_open_ex: unknown flag bits 0x6 (known: WS_STREAM_BLOCK_KERNEL = 1)" in E.lib().ws_engine_last_error().decode()
    assert not h.value
    assert E.lib().ws_engine_pool_open_ex(eng._h, 2, G, 3, ctypes.byref(h)) == -1
    assert "ws_engine_pool_open_ex: unknown flag bits 0x2 (known: WS_STREAM_BLOCK_KERNEL = 1)" in E.lib().ws_engine_last_error().decode()
    assert not h.value
    assert E.lib().ws_engine_pool_open_ex(eng._h, 2, G, 0, ctypes.byref(h)) == 0 and h.value      # flags = 0 is the plain open
    E.lib().ws_engine_pool_close(h)
    with pytest.raises(E.WesepHipError, match="slots=0, a pool has at least one"):                # the plain open's refusals stay
        eng.stream_pool(0, block_kernel=True)
    eng.close()
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    gpath = str(tmp_path / "g.wsw")
    export_engine(get_model("ConvTasNet")(**dict(KW, joint_training=False)), gpath)
    geng = E.Engine(gpath, dry_run=True)
    with pytest.raises(E.WesepHipError, match="ws_engine_stream_open: this Conv-TasNet container is non-causal with gLN"):
        geng.stream(2, emb, E.ENROLL_EMBEDDING, block_kernel=True)
    geng.close()


@needs_no_gpu
def test_separate_main_stream_block_dry_run_and_refusal(tmp_path):
    exe = os.path.join(ROOT, "runtime", "separate_main")
    model = _export(tmp_path, joint=True, N=256)
    rng = np.random.default_rng(1)
    lines, lens = [], {"u1": 3203, "u2": 1600, "u3": 170}
    for key, n in lens.items():
        _write_wav(tmp_path / f"{key}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"{key}_e1.wav", rng.integers(-3000, 3000, 900))
        _write_wav(tmp_path / f"{key}_e2.wav", rng.integers(-3000, 3000, 1000))
        lines.append(f"{key} {tmp_path}/{key}.wav {tmp_path}/{key}_e1.wav {tmp_path}/{key}_e2.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    run = lambda *a: subprocess.run([exe, "--wav_scp", str(scp), "--dry_run", "--model", model, *a], capture_output=True, text=True,
                                    timeout=120)
    r = run("--stream_ms", "10", "--stream_block")
    assert r.returncode == 0, r.stderr
    for key, n in lens.items():
        assert f"process: {key} RTF:" in r.stdout and f"({-(-n // 160)} pushes of 160 samples" in r.stdout, r.stdout
    r = run("--stream_ms", "10", "--stream_block", "--stream_pool", "3")
    assert r.returncode == 0, r.stderr
    count = lambda out: tuple(int(v) for v in out.split("pool: ")[1].split(" launches")[0].split(" rounds, "))
    rounds, launches = count(r.stdout)
    plain = run("--stream_ms", "10", "--stream_pool", "3")
    rounds0, launches0 = count(plain.stdout)
    groups = launches0 // (3 * RX + 9)                               # the same groups, WS_POOL_BLOCK_GROUP_LAUNCHES each
    assert rounds == rounds0 and launches0 == groups * (3 * RX + 9) and launches == groups * (RX + 9) and groups >= rounds
    r = run("--stream_block")
    assert r.returncode == 1 and "--stream_block needs --stream_ms" in r.stderr
    r = run("--stream_block", "--stream_pool", "3")
    assert r.returncode == 1 and ("--stream_pool needs --stream_ms" in r.stderr or "--stream_block needs --stream_ms" in r.stderr)
