"""ovo_amd.build rebuilds exactly what changed: an object is stale when a source is newer OR when it was compiled by another command line (no GPU, no hipcc:
the compiler call is stubbed and the output directory is a temporary one)."""
import os


def test_a_changed_flag_rebuilds_its_object_and_relinks(tmp_path, monkeypatch):
    from ovo_amd import build as B
    out = tmp_path / "lib"
    monkeypatch.setattr(B, "OUT_DIR", str(out))
    monkeypatch.setattr(B, "OBJ_DIR", str(out / "obj"))
    monkeypatch.setattr(B, "SO", str(out / "libovo_hip.so"))
    monkeypatch.delenv("OVO_HIPCC_EXTRA", raising=False)
    ran = []

    def fake_run(cmd, what):
        target = cmd[cmd.index("-o") + 1]
        ran.append((os.path.basename(target), cmd))
        with open(target, "w") as f:
            f.write("x")

    monkeypatch.setattr(B, "_run", fake_run)

    def step(**kw):
        ran.clear()
        B.build(verbose=False, **kw)
        ran[:-1] = sorted(ran[:-1])                                            # objects compile in parallel; the link comes last
        return [name for name, _ in ran]

    everything = sorted(s.replace(".hip", ".o") for s in B.sources()) + ["libovo_hip.so"]
    assert len(everything) > 10
    assert step() == everything                                                # every object, then the link
    assert step() == []                                                        # nothing changed: nothing runs
    monkeypatch.setenv("OVO_HIPCC_EXTRA", "query.hip=-DOVO_DUMMY")
    assert step() == ["query.o", "libovo_hip.so"]
    assert "-DOVO_DUMMY" in ran[0][1] and "-DOVO_DUMMY" not in ran[1][1]
    assert step() == []
    monkeypatch.delenv("OVO_HIPCC_EXTRA")
    assert step() == ["query.o", "libovo_hip.so"]
    assert "-DOVO_DUMMY" not in ran[0][1]
    # the build's options are flags like any other, and leave the module's own table alone
    extra = {f: list(v) for f, v in B.EXTRA.items()}
    assert step(gemm_debug=True) == ["gemm8p.o", "gemm8q.o", "libovo_hip.so"]
    assert step(gemm_debug=True) == []
    assert step(experimental=True) == ["gemm8p.o", "gemm8q.o", "geometry.o", "libovo_hip.so"]
    assert step() == ["gemm8q.o", "geometry.o", "libovo_hip.so"]
    assert B.EXTRA == extra
    assert step(force=True)[-1] == "libovo_hip.so" and len(ran) == len(everything)
