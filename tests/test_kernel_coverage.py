"""Every mh_* entry point declared in include/memehip.h is exercised by a GPU test module, by name or through the ops.py wrapper
that calls it, or is on the short allowlist below with the reason it needs no kernel test.  A new export without a test fails
here, on the CPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALLOWLIST = {
    "mh_status_str": "host-only: maps a status code to its message",
    "mh_gemm_set_trace": "profiling switch of tools/gemm_timeline.py; stores a pointer, launches nothing",
    "mh_gemm_ksplit_for": "host-only arithmetic: the split-K chunk count",
    "mh_bn2d_workspace_elems": "host-only workspace-size query",
    "mh_version": "host-only: the library's version word",
}


def _declared():
    text = open(os.path.join(ROOT, "include", "memehip.h"), encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|void|const char\s*\*)\s+(mh_\w+)\s*\(", text, flags=re.M)))


def _wrappers():
    """ops.py function name -> the mh_* entry points its body calls"""
    src = open(os.path.join(ROOT, "multimodal_propaganda_meme_classification_amd", "ops.py"), encoding="utf-8").read()
    out = {}
    for m in re.finditer(r"^def (\w+)\(.*?(?=^def |\Z)", src, flags=re.M | re.S):
        out[m.group(1)] = set(re.findall(r"\.(mh_\w+)\(", m.group(0)))
    return out


def _gpu_test_text():
    texts = []
    for path in glob.glob(os.path.join(ROOT, "tests", "test_*.py")):
        t = open(path, encoding="utf-8").read()
        if "mark.gpu" in t:
            texts.append(t)
    return "\n".join(texts)


def test_every_export_has_a_gpu_test():
    declared = _declared()
    assert len(declared) > 50, declared
    text = _gpu_test_text()
    called = set()
    for fn, entries in _wrappers().items():
        if re.search(r"\bops\.%s\(" % fn, text):
            called |= entries
    missing = [n for n in declared if n not in ALLOWLIST and n not in called and not re.search(r"\b%s\b" % n, text)]
    assert not missing, f"exported without a GPU test (add one, or an ALLOWLIST entry with its reason): {missing}"
    stale = [n for n in ALLOWLIST if n not in declared]
    assert not stale, f"ALLOWLIST names entry points the header no longer declares: {stale}"
