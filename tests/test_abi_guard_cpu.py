"""CPU: no C++ exception crosses the C ABI of libcvxalign.so.  Every cvx_* entry defined in ngmlr_amd/csrc/*.cpp that returns a
status (int) opens with ABI_GUARD_BEGIN as its first statement and closes with ABI_GUARD_END (cvx_rt_err.h), or is a
function-try-block; every one that returns nothing opens with ABI_GUARD_BEGIN and closes with ABI_GUARD_END_VOID.  Checked on the
sources, so that whether an entry is covered never has to be worked out from its call chain: a std::bad_alloc that reaches the
ABI terminates the caller (ngmlr) instead of returning a status."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngmlr_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "cvx_align.h")
# returns a constant.  (The other accessors that need no guard -- cvx_last_error, cvx_build_id, cvx_source_id,
# cvx_genome_encoded_bytes -- return neither a status nor nothing, so the check does not look at them.)
UNGUARDED = {"cvx_abi_version"}


def _code(path):
    """the file without its comments, every string and character literal emptied"""
    def blank(m):
        s = m.group(0)
        return '""' if s[0] == '"' else "''" if s[0] == "'" else " "
    return re.sub(r'/\*.*?\*/|//[^\n]*|"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'', blank, open(path).read(), flags=re.S)


def _definitions(code):
    """(return type, name, text from the end of the parameter list on) of every definition of an int or void cvx_* function"""
    for m in re.finditer(r'^[ \t]*(?:extern\s*""\s*)?(?:static\s+)?(int|void)\s+(cvx_\w+)\s*\(', code, re.M):
        i, depth = m.end() - 1, 0
        while True:
            depth += {"(": 1, ")": -1}.get(code[i], 0)
            if depth == 0:
                break
            i += 1
        rest = code[i + 1:].lstrip()
        if rest.startswith("{") or re.match(r"try\b", rest):
            yield m.group(1), m.group(2), rest


def _body(rest):
    depth = 0
    for j, c in enumerate(rest):
        depth += {"{": 1, "}": -1}.get(c, 0)
        if depth == 0:
            return rest[1:j]


def test_no_exception_crosses_the_c_abi():
    seen, bad = set(), []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.cpp"))):
        for ret, name, rest in _definitions(_code(path)):
            seen.add(name)
            if name in UNGUARDED or re.match(r"try\b", rest):
                continue
            body = _body(rest).strip()
            end = "ABI_GUARD_END" if ret == "int" else "ABI_GUARD_END_VOID"
            if not re.match(r"ABI_GUARD_BEGIN\b", body) or not re.search(r"\b%s$" % end, body):
                bad.append("%s (%s)" % (name, os.path.basename(path)))
    assert not bad, "a C++ exception can leave these entries: " + ", ".join(bad)
    # every int / void entry of the public header was looked at (a definition the pattern missed would pass unchecked)
    declared = set(re.findall(r"^(?:int|void)\s+(cvx_\w+)\s*\(", open(HEADER).read(), re.M))
    assert len(declared) > 50 and declared <= seen, sorted(declared - seen)
