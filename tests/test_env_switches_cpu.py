"""The shipped package reads no environment variable that selects between two implementations of the same result: A/B runs build the
other version and load it through MAAVSS_LIB (scripts/ab_step.py, scripts/*_bench.py).  This test lists every MAAVSS_* name that the
Python package and the HIP sources read from the environment and compares the set with the allow-list below, so that a new run-time
switch has to be argued for here.  Source text only: no GPU, no compiler."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALLOWED = {
    "MAAVSS_QKV_LN": "default of the constructor argument VideoAttention(qkv_ln=...), pinned by tests/test_vit_base_cpu.py",
    "MAAVSS_WGRAD_X16": "documented opt-in (README.md): bf16 copies of the activations for the weight-gradient kernels",
    "MAAVSS_ATTN_ABL": "inside #ifdef MAAVSS_ATTN_ABLATE: measurement build (make ablate) only, not in the shipped library",
}

# os.environ.get("X"), os.environ["X"], os.environ.pop / setdefault("X"), os.getenv("X"), getenv("X"), "X" in os.environ
_READS = (re.compile(r"""(?:\benviron\s*(?:\.\s*\w+\s*\(|\[)|\bgetenv\s*\()\s*["'](MAAVSS_\w+)["']"""),
          re.compile(r"""["'](MAAVSS_\w+)["']\s+(?:not\s+)?in\s+(?:os\s*\.\s*)?environ\b"""))


def env_names(root):
    pkg = os.path.join(root, "maavss_amd")
    files = glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True)
    files += glob.glob(os.path.join(pkg, "csrc", "*.hip")) + glob.glob(os.path.join(pkg, "csrc", "*.h"))
    found = {}
    for path in files:
        with open(path, encoding="utf-8") as fh:
            text = fh.read()
        for rx in _READS:
            for name in rx.findall(text):
                found.setdefault(name, set()).add(os.path.relpath(path, root))
    return found


def test_the_scan_sees_every_spelling_of_an_environment_read(tmp_path):
    csrc = tmp_path / "maavss_amd" / "csrc"
    csrc.mkdir(parents=True)
    (tmp_path / "maavss_amd" / "a.py").write_text(
        'import os\na = os.environ.get("MAAVSS_A", "1")\nb = os.environ["MAAVSS_B"]\nc = os.getenv(\'MAAVSS_C\')\n'
        'd = "MAAVSS_D" in os.environ\ne = os.environ.pop("MAAVSS_E", None)\n# MAAVSS_COMMENT is only named\n')
    (csrc / "k.hip").write_text('static const bool f = getenv("MAAVSS_F") != nullptr;\n#ifdef MAAVSS_MACRO\n#endif\n')
    (csrc / "k.h").write_text('const char* g = std::getenv( "MAAVSS_G" );\n')
    assert set(env_names(str(tmp_path))) == {"MAAVSS_" + c for c in "ABCDEFG"}


def test_environment_switches_are_the_allow_list():
    found = env_names(ROOT)
    extra = {n: sorted(f) for n, f in found.items() if n not in ALLOWED}
    assert not extra, ("new environment switch(es) in the shipped package: %r -- A/B another build through MAAVSS_LIB instead, or add the "
                       "name to ALLOWED with the reason it stays" % extra)
    gone = sorted(set(ALLOWED) - set(found))
    assert not gone, "no longer read anywhere, remove from ALLOWED: %r" % gone
