"""gs360_MaskFinish's argument handling: the reference's checks and messages, the two stages that are not built and the missing
directories.  All of these end before a context is made, so they need no GPU."""
import pytest

import gs360_MaskFinish as tool


def run(capsys, argv):
    rc = tool.main(argv)
    out = capsys.readouterr()
    return rc, out.out, out.err


@pytest.fixture()
def folders(tmp_path):
    (tmp_path / "in").mkdir()
    (tmp_path / "raw").mkdir()
    return tmp_path


def test_defaults_are_the_references():
    a = tool.create_arg_parser().parse_args(["-i", "x"])
    assert (a.mode, a.close, a.mask_expand_mode, a.mask_expand_pixels, a.mask_expand_percent, a.edge_fuse_pixels) == ("mask", 5, "pixels", 15, 1.0, 25)
    assert a.out is None and a.raw_mask_dir is None and a.manual_mask_dir is None and not a.include_shadow


@pytest.mark.parametrize("flag", ["--mask-expand-pixels", "--mask-expand-percent", "--edge-fuse-pixels"])
def test_negative_amounts_are_parser_errors(capsys, folders, flag):
    with pytest.raises(SystemExit) as e:
        tool.main(["-i", str(folders / "in"), "--raw-mask-dir", str(folders / "raw"), flag, "-1"])
    assert e.value.code == 2 and f"{flag} must be 0 or greater" in capsys.readouterr().err


def test_unknown_mode_and_expand_mode_are_parser_errors(folders):
    for extra in (["--mode", "blur"], ["--mask-expand-mode", "ratio"]):
        with pytest.raises(SystemExit) as e:
            tool.main(["-i", str(folders / "in")] + extra)
        assert e.value.code == 2


@pytest.mark.parametrize("extra, word", [(["--mode", "inpaint"], "inpainting"), (["--include_shadow"], "shadow estimate")])
def test_the_stages_that_are_not_built_end_the_run_with_one_err_line(capsys, folders, extra, word):
    rc, out, _err = run(capsys, ["-i", str(folders / "in"), "--raw-mask-dir", str(folders / "raw")] + extra)
    lines = out.splitlines()
    assert rc == 1 and len(lines) == 1 and lines[0].startswith("[ERR] ") and "not built" in lines[0] and word in lines[0]


def test_without_masks_of_either_kind_the_network_is_named(capsys, folders):
    rc, out, _err = run(capsys, ["-i", str(folders / "in")])
    lines = out.splitlines()
    assert rc == 1 and len(lines) == 1 and lines[0].startswith("[ERR] ") and "network is not part of this build" in lines[0]


def test_missing_directories(capsys, folders):
    rc, _out, err = run(capsys, ["-i", str(folders / "nope"), "--raw-mask-dir", str(folders / "raw")])
    assert rc == 1 and err.strip() == f"Input directory not found: {folders / 'nope'}"
    rc, _out, err = run(capsys, ["-i", str(folders / "in"), "--manual-mask-dir", str(folders / "paint")])
    assert rc == 1 and err.strip() == f"Manual mask directory not found: {folders / 'paint'}"
    rc, _out, err = run(capsys, ["-i", str(folders / "in"), "--raw-mask-dir", str(folders / "none")])
    assert rc == 1 and err.strip() == f"Raw mask directory not found: {folders / 'none'}"


def test_an_empty_input_folder(capsys, folders):
    (folders / "in" / "notes.txt").write_text("no image")
    rc, out, err = run(capsys, ["-i", str(folders / "in"), "--raw-mask-dir", str(folders / "raw"), "--mask-expand-mode", "percent"])
    assert rc == 1 and err.strip() == "No images found."
    assert out.splitlines() == ["Mask expand: 1.0%", "Edge fuse: 25 px"]
