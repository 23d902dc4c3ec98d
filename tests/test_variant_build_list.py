"""tools/build_variant.sh links the translation units the product Makefile lists: a unit added to the library must not be
missing from the variant libraries (they would link, with undefined symbols, and fail to load)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flashattention_kernel_project_amd", "csrc")


def test_variant_script_takes_its_sources_from_the_makefile():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.+)$", makefile, re.M).group(1).split()
    assert "fa_fwd_kvcache.hip" in srcs and "fa_capi.hip" in srcs
    script = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    line = re.search(r"^SRCS=\$\((.+)\)$", script, re.M)
    assert line, "build_variant.sh must derive SRCS from the Makefile"
    got = subprocess.run(["bash", "-c", f'src="{CSRC}"; {line.group(1)}'], capture_output=True, text=True, check=True).stdout.split()
    assert got == srcs
    # and it names no translation unit the Makefile does not have
    for name in re.findall(r"\bfa_\w+\.hip\b", script):
        assert name in srcs, name
