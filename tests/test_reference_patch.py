"""The reference-side change that makes `linsolve = :hipldl` selectable (row b of SURVEY 8: the drop-in boundary).

`cannoles.jl_amd/julia/cannoles_hipldl.patch` is the diff a maintainer applies to CaNNOLeS.jl.  The tests read the patch itself
and `tests/golden/reference_patch.json`, facts recorded from the unpatched CaNNOLeS.jl the patch is written against (line counts,
sha256 of the lines every hunk replaces, where the backend selection of `CaNNOLeSSolver` sits, which guards and branches it has).
They check that
  * the patch applies cleanly: every hunk is well-formed and its pre-image is, line for line, what the reference holds at that
    place (no offset, no fuzz), and a new file is new,
  * on an install WITHOUT HSL — the normal case — `linsolve = :hipldl` reaches the new branch of the if-chain: every
    guard in front of the chain (src/CaNNOLeS.jl:317-320 rewrites any backend other than `:ldlfactorizations` when HSL is
    not functional) is evaluated for that case,
  * element types other than Float64 and sessions without CaNNOLeSHIP fall back to `:ldlfactorizations`,
  * `:ma57` without HSL still falls back as before,
  * the extension file inside the patch is the one shipped under cannoles.jl_amd/julia/ext/.
No Julia is executed (there is none in the image): the guards are simple boolean expressions over `linsolve`, `T`,
`LIBHSL_isfunctional()` and `hipldl_available(...)`, translated to Python here.

`python tests/test_reference_patch.py <CaNNOLeS.jl checkout>` records the fixture again.
"""
import hashlib
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "cannoles.jl_amd", "julia", "cannoles_hipldl.patch")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_patch.json")
MAIN = "src/CaNNOLeS.jl"
GUARD = r"(?m)^  if (.+)\n((?:    .*\n)+?)  end$"
BRANCH = r"(?:if|elseif) linsolve == :([a-z0-9_]+)\n((?:    .*\n)+)"


class Hunk:
    def __init__(self, old_start, old_len, new_start, new_len):
        self.old_start, self.old_len, self.new_start, self.new_len = old_start, old_len, new_start, new_len
        self.lines = []   # (tag, text), tag in " -+"

    def image(self, which):
        """the hunk's lines before ("old") or after ("new") the patch, each ending in a newline"""
        keep = " -" if which == "old" else " +"
        return "".join(t + "\n" for tag, t in self.lines if tag in keep)

    @property
    def key(self):
        return f"{self.old_start},{self.old_len}"


def parse_patch(path=PATCH):
    """{file: [Hunk]} of a unified diff; every hunk must hold exactly the lines its header counts"""
    files, lines, i = {}, open(path).read().split("\n"), 0
    while i < len(lines):
        ln = lines[i]
        i += 1
        if ln.startswith("+++ "):
            name = ln[4:].split("\t")[0]
            cur = files.setdefault(name[2:] if name.startswith("b/") else name, [])
            continue
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", ln)
        if not m:
            continue
        h = Hunk(int(m.group(1)), int(m.group(2) or 1), int(m.group(3)), int(m.group(4) or 1))
        old = new = 0
        while old < h.old_len or new < h.new_len:
            ln = lines[i]
            i += 1
            tag = ln[:1] or " "
            assert tag in " -+", f"malformed hunk {h.key}: {ln!r}"
            h.lines.append((tag, ln[1:]))
            old += tag in " -"
            new += tag in " +"
        assert (old, new) == (h.old_len, h.new_len), f"hunk {h.key}: counts do not match its header"
        if i < len(lines) and lines[i].startswith("\\"):
            i += 1
        cur.append(h)
    return files


def _sha(lines):
    return hashlib.sha256("".join(t + "\n" for t in lines).encode()).hexdigest()


def record(ref):
    """the fixture, from an unpatched CaNNOLeS.jl checkout at `ref` (facts about its text, none of the text itself)"""
    rec = {"files": {}}
    for name, hunks in parse_patch().items():
        path = os.path.join(ref, name)
        if not os.path.exists(path):
            rec["files"][name] = {"exists": False}
            continue
        src = open(path).read().split("\n")[:-1]
        rec["files"][name] = {"exists": True, "lines": len(src),
                              "hunk_sha256": {h.key: _sha(src[h.old_start - 1:h.old_start - 1 + h.old_len]) for h in hunks}}
    src = open(os.path.join(ref, MAIN)).read()
    line = lambda pos: src.count("\n", 0, pos) + 1   # noqa: E731
    start = src.index("function CaNNOLeSSolver(")
    chain = src.index("LDLT = if linsolve == :ma57", start)
    end = src.index("F = typeof(LDLT)", chain)
    kw = src.index("# Keyword arguments")
    rec["constructor"] = {
        "file": MAIN, "start": line(start), "chain": line(chain), "end": line(end),
        "guards_on_linsolve": [line(start + m.start()) for m in re.finditer(GUARD, src[start:chain]) if "linsolve" in m.group(1)],
        "chain_branches": [sym for sym, _ in re.findall(BRANCH, src[chain:end])],
        "keyword_docs": [line(kw), line(src.index("max_iter::Int", kw))]}
    return rec


def _fixture():
    return json.load(open(FIXTURE))


def _backend_selection(which):
    """(guards, branches) of the backend selection of CaNNOLeSSolver before ("old") or after ("new") the patch: the guards on
    `linsolve` in front of the if-chain [(condition, body)] and the branches of the chain [(symbol, body)].  Every guard of the
    unpatched constructor lies inside a hunk, so the hunks' images hold all guards of either version; the chain's branches are
    the recorded ones, less those a hunk removes, plus those a hunk adds (with their bodies)."""
    rec = _fixture()["constructor"]
    hunks = parse_patch()[rec["file"]]
    front = [h for h in hunks if h.old_start < rec["chain"] and h.old_start + h.old_len > rec["start"]]
    for g in rec["guards_on_linsolve"]:
        assert any(h.old_start <= g < h.old_start + h.old_len for h in front), f"guard at line {g} outside every hunk"
    guards = [(c, b) for h in front for c, b in re.findall(GUARD, h.image(which)) if "linsolve" in c]
    old_guards = [(c, b) for h in front for c, b in re.findall(GUARD, h.image("old")) if "linsolve" in c]
    assert len(old_guards) == len(rec["guards_on_linsolve"]), "a hunk cuts a guard"
    inside = [h for h in hunks if rec["chain"] < h.old_start < rec["end"]]
    before = dict(b for h in inside for b in re.findall(BRANCH, h.image("old")))
    after = dict(b for h in inside for b in re.findall(BRANCH, h.image(which)))
    branches = [(sym, "") for sym in rec["chain_branches"] if sym in after or sym not in before]
    branches += [(sym, body) for sym, body in after.items() if sym not in rec["chain_branches"]]
    return guards, branches


def _added(hunks):
    """(line of the unpatched file in front of which it goes, text) of every added line"""
    out = []
    for h in hunks:
        at = h.old_start
        for tag, text in h.lines:
            if tag == "+":
                out.append((at, text))
            else:
                at += 1
    return out


def _post_image(name):
    return "".join(h.image("new") for h in parse_patch()[name])


def _julia_cond_to_python(cond):
    c = cond
    c = re.sub(r":([A-Za-z_][A-Za-z_0-9]*)", r"'\1'", c)          # Symbols
    c = c.replace("&&", " and ").replace("||", " or ")
    c = re.sub(r"!(?!=)", " not ", c)                               # `!x`, `!(…)`; `!=` stays
    c = re.sub(r"hipldl_available\([^)]*\)", "HIPLDL", c)
    c = c.replace("LIBHSL_isfunctional()", "HSL")
    return c


def _selected_backend(which, linsolve, T, hsl, ext_loaded):
    """Walk the guards in front of the if-chain and then the chain itself, as Julia would."""
    guards, branches = _backend_selection(which)
    for cond, body in guards:
        m = re.search(r"\n?\s*linsolve = :([a-z0-9_]+)", body)
        assert m, f"guard on linsolve that does not reassign it: {cond}"
        env = {"linsolve": linsolve, "T": T, "Float64": "Float64", "HSL": hsl, "HIPLDL": ext_loaded}
        if eval(_julia_cond_to_python(cond), {}, env):
            linsolve = m.group(1)
    for sym, body in branches:
        if sym == linsolve:
            return sym, body
    return None, ""


def test_patch_applies_and_extension_file_is_the_shipped_one():
    rec = _fixture()
    patch = parse_patch()
    assert set(patch) == set(rec["files"]), (sorted(patch), sorted(rec["files"]))
    for name, hunks in patch.items():
        f = rec["files"][name]
        if not f["exists"]:   # a new file: one hunk, all of it added
            assert len(hunks) == 1 and (hunks[0].old_start, hunks[0].old_len) == (0, 0), name
            assert all(tag == "+" for tag, _ in hunks[0].lines), name
            continue
        last = 0
        for h in hunks:   # in order, inside the file, and the lines each hunk replaces are the reference's at that place
            assert last < h.old_start and h.old_start + h.old_len - 1 <= f["lines"], (name, h.key)
            assert f["hunk_sha256"].get(h.key) == _sha([t for tag, t in h.lines if tag in " -"]), f"{name} {h.key} does not apply"
            last = h.old_start + h.old_len - 1
    shipped = open(os.path.join(ROOT, "cannoles.jl_amd", "julia", "ext", "CaNNOLeSHIPExt.jl")).read()
    assert _post_image("ext/CaNNOLeSHIPExt.jl") == shipped
    proj = _post_image("Project.toml")
    assert "[weakdeps]" in proj and "[extensions]" in proj and 'CaNNOLeSHIPExt = "CaNNOLeSHIP"' in proj
    uuid = re.search(r'uuid = "([0-9a-f-]+)"', open(os.path.join(ROOT, "cannoles.jl_amd", "julia", "CaNNOLeSHIP", "Project.toml")).read()).group(1)
    assert f'CaNNOLeSHIP = "{uuid}"' in proj
    types = _post_image("src/solver_types.jl")
    assert "function linear_solver_struct end" in types and "hipldl_available(rows, cols, vals) = hasmethod(" in types
    kw0, kw1 = rec["constructor"]["keyword_docs"]   # the keyword arguments of the docstring: `:hipldl` is added between these lines
    assert any(kw0 < at <= kw1 for at, text in _added(patch[MAIN]) if "`:hipldl`" in text)


def test_hipldl_reaches_its_branch_without_hsl():
    sym, body = _selected_backend("new", "hipldl", "Float64", hsl=False, ext_loaded=True)
    assert sym == "hipldl"
    assert "linear_solver_struct(Val(:hipldl), nvar + nequ + ncon, rows, cols, vals, nvar, nequ, ncon)" in body
    assert "vals = get_vals(LDLT)" in body          # solver.vals stays the array the backend holds (CaNNOLeS.jl:324,328)
    # and with HSL present as well
    assert _selected_backend("new", "hipldl", "Float64", hsl=True, ext_loaded=True)[0] == "hipldl"


def test_unpatched_reference_reroutes_hipldl():
    """The finding this patch answers: in the reference as it stands the guard at src/CaNNOLeS.jl:317-320 turns any backend
    other than :ldlfactorizations into :ldlfactorizations when HSL is missing — a branch added to the chain alone is dead."""
    assert _selected_backend("old", "hipldl", "Float64", hsl=False, ext_loaded=True)[0] == "ldlfactorizations"


@pytest.mark.parametrize("T,ext", [("Float32", True), ("Float16", True), ("BigFloat", True), ("Float64", False)])
def test_fallback_to_the_cpu_backend(T, ext):
    # the reference's test/runtests.jl:102-113 runs Float16/32/BigFloat: those must stay on LDLFactStruct
    assert _selected_backend("new", "hipldl", T, hsl=False, ext_loaded=ext)[0] == "ldlfactorizations"
    assert _selected_backend("new", "hipldl", T, hsl=True, ext_loaded=ext)[0] == "ldlfactorizations"


def test_other_backends_unchanged():
    assert _selected_backend("new", "ma57", "Float64", hsl=False, ext_loaded=True)[0] == "ldlfactorizations"
    assert _selected_backend("new", "ma57", "Float64", hsl=True, ext_loaded=True)[0] == "ma57"
    assert _selected_backend("new", "ldlfactorizations", "Float64", hsl=False, ext_loaded=False)[0] == "ldlfactorizations"
    assert _selected_backend("new", "foo", "Float64", hsl=True, ext_loaded=True)[0] is None      # error("Can't handle …")


if __name__ == "__main__":
    json.dump(record(sys.argv[1]), open(FIXTURE, "w"), indent=1)
    open(FIXTURE, "a").write("\n")
