"""CPU: jnn --segmenter, prefix --adaptor, prefix --polya on the command line (no GPU needed): malformed lists and values
outside the domain end with a message and exit 1 before any file is opened, the options belong to their subtools, and the
list parsers run clean under the address and undefined-behaviour sanitizers in a stand-alone program."""
import os
import shutil
import subprocess

import pytest

from sigtk_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOFILE = "/nonexistent/reads.blow5"


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI):
        build.build_lib()
        build.build_cli()
    return build.CLI


def _run(cli, *args):
    return subprocess.run([cli, *args, NOFILE], capture_output=True, text=True)


BAD = {
    ("jnn", "--segmenter"): [
        "", ",", "0.75,50,50,150,0.25", "0.75,50,50,150,0.25,5,1,2", "-1,50,200,250,1,30", "-1,50,200,250,1,30,560",
        "-1,50,200,250,1,30,560,420,1", "0.75,,50,150,0.25,5", "0.75,50,50,150,0.25,5,", "0.75, 50,50,150,0.25,5",
        "0.75,50x,50,150,0.25,5", "0.75,50.0,50,150,0.25,5", "0.75,50,50,150,0.25,5 ", "abc",
        # out of domain
        "0.75,50,50,31,0.25,5", "0.75,50,50,16777217,0.25,5", "0.75,0,50,150,0.25,5", "0.75,50,-1,150,0.25,5",
        "0.75,50,50,150,-0.25,5", "0.75,50,50,150,0.25,-1", "0.75,50,50,150,nan,5", "inf,50,50,150,0.25,5",
        "nan,50,50,150,0.25,5,1,2", "0.75,50,50,99999999999,0.25,5"],
    ("prefix", "--adaptor"): [
        "", "0.5,1500,2000,200000", "0.5,1500,2000,200000,2000,1", "0.5,1500,2000.0,200000,2000", "0.5,1500,2000,200000,2000 ",
        "0.5,,2000,200000,2000", "x",
        "0.5,1500,1,200000,2000", "0.5,1500,13982,200000,2000", "0.5,1500,2000,200000,0", "0.5,1500,2000,1999,2000",
        "0.5,-1,2000,200000,2000", "nan,1500,2000,200000,2000", "inf,1500,2000,200000,2000"],
    ("prefix", "--polya"): [
        "", "50,200,250,1,30,30", "50,200,250,1,30,30,20,1", "50.5,200,250,1,30,30,20", "50,200,250,1,30,30,20 ", "50,200,,1,30,30,20",
        "50,200,31,1,30,30,20", "0,200,250,1,30,30,20", "50,-1,250,1,30,30,20", "50,200,250,-1,30,30,20", "50,200,250,1,-1,30,20",
        "50,200,250,1,30,nan,20", "50,200,250,1,30,30,-1", "50,200,250,1,30,30,inf", "50,200,250,nan,30,30,20"],
}


@pytest.mark.parametrize("tool,option,arg", [(t, o, a) for (t, o), args in BAD.items() for a in args])
def test_cli_refuses_a_bad_list(cli, tool, option, arg):
    p = _run(cli, tool, option, arg)
    assert p.returncode == 1, (arg, p.stderr)
    assert option in p.stderr and "cannot open" not in p.stderr and p.stdout == "", (arg, p.stderr)


@pytest.mark.parametrize("tool,option,arg", [
    ("jnn", "--segmenter", "0.75,50,50,150,0.25,5"), ("jnn", "--segmenter", "-1,50,200,250,1,30,nan,420"),
    ("jnn", "--segmenter", "0.6,17,30,32,0.5,40"), ("prefix", "--adaptor", "0.5,1500,2,200000,1"),
    ("prefix", "--adaptor", "0.7,0,13981,5,5"), ("prefix", "--polya", "50,200,250,0.5,50,-3.5,0")])
def test_cli_takes_a_good_list_as_far_as_the_file(cli, tool, option, arg):
    p = _run(cli, tool, option, arg)
    assert p.returncode == 1 and "cannot open" in p.stderr, p.stderr
    assert "unrecognized option" not in p.stderr and option not in p.stderr, p.stderr     # the list itself was taken


def test_options_belong_to_their_subtools(cli):
    good = {"--segmenter": "0.75,50,50,150,0.25,5", "--adaptor": "0.5,1500,2000,200000,2000", "--polya": "50,200,250,1,30,30,20"}
    owner = {"--segmenter": "jnn", "--adaptor": "prefix", "--polya": "prefix"}
    for option, arg in good.items():
        for tool in ("pa", "event", "stat", "jnn", "prefix", "ent", "qts", "sref", "ss"):
            if tool == owner[option]:
                continue
            p = _run(cli, tool, option, arg)
            # (qts, sref and ss parse their own options: there the option does not exist at all)
            refused = "unrecognized option" in p.stderr if tool in ("qts", "sref", "ss") else p.returncode == 1 and option in p.stderr
            assert refused and "cannot open" not in p.stderr and "Error in opening" not in p.stderr, (tool, option, p.stderr)
    for tool, option in (("jnn", "--segmenter"), ("prefix", "--adaptor"), ("prefix", "--polya")):
        p = subprocess.run([cli, tool, "-h"], capture_output=True, text=True)
        assert p.returncode == 0 and option in p.stdout
    p = subprocess.run([cli, "stat", "-h"], capture_output=True, text=True)
    assert p.returncode == 0 and "--segmenter" not in p.stdout and "--adaptor" not in p.stdout


def test_list_parsers_under_the_sanitizers(tmp_path):
    """tools/segopt_check.c: a program of its own with its own main, built with -fsanitize=address,undefined"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "segopt_check")
    subprocess.check_call([cc, "-O1", "-g", "-std=c99", "-D_GNU_SOURCE", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tools", "segopt_check.c")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 wrong" in p.stdout
