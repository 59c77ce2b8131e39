"""csrc/tree_shape.h -- heights, levels, min / max indices and roots of a binary forest, and ryhope's sbbst -- compiled for the host
under -fsanitize=address,undefined (tools/hosttest/tree_shape_test.cpp, a stand-alone program) and held against the Python
restatements of tests/tree_cases.py: table.py's sbbst for every n in 0..70, balanced BSTs, the BST of a random insertion order, left
and right chains, a forest of three trees; a chain of 2^20 nodes (shape only: the case that catches recursion); and the malformed
children arrays, each refused with a message and a clean exit. Exit status 0 and an empty stderr throughout."""
import subprocess

import pytest

import hosttest
import tree_cases as TC


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = hosttest.build(tmp_path_factory.mktemp("tree_shape"), "tree_shape_test",
                         flags=("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), mp2g_h=False)

    def go(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stdout[-300:] + r.stderr[-2000:]
        return r.stdout.splitlines()
    return go


def tree_line(left, right):
    return f"tree {len(left)} " + " ".join(f"{l} {r}" for l, r in zip(left, right))


def parse_shape(lines):
    """the nine lines of an accepted shape -> (levels, {name: numbers})"""
    assert lines[0].split()[0] == "ok", lines[0]
    out = {}
    for name, ln in zip(("left", "right", "height", "min", "max", "roots", "order", "off"), lines[1:9]):
        t = ln.split()
        assert t[0] == name, ln
        out[name] = [int(x) for x in t[1:]]
    return int(lines[0].split()[1]), out


def check(left, right, levels, s):
    TC.check_shape(left, right, s["left"], s["right"], s["height"], s["min"], s["max"], s["roots"])
    n = len(left)
    assert levels == (max(s["height"]) + 1 if n else 0) and len(s["off"]) == levels + 1
    assert s["off"][0] == 0 and s["off"][-1] == n and sorted(s["order"]) == list(range(n))
    for h in range(levels):  # level h = exactly the nodes of height h, in ascending order
        level = s["order"][s["off"][h]:s["off"][h + 1]]
        assert level == [i for i in range(n) if s["height"][i] == h]


def test_sbbst_is_table_py(run):
    ns = list(range(0, 71))
    lines = run("\n".join(f"sbbst {n}" for n in ns))
    assert len(lines) == 10 * len(ns)
    for j, n in enumerate(ns):
        chunk = lines[10 * j:10 * j + 10]
        assert chunk[0] == f"sbbst {TC.T.sbbst_root(n)}"
        levels, s = parse_shape(chunk[1:])
        left, right = TC.sbbst(n)
        check(left, right, levels, s)
        assert s["roots"] == ([TC.T.sbbst_root(n) - 1] if n else [])


def test_accepted_shapes(run):
    cases = TC.accepted(small=False)
    lines = run("\n".join(tree_line(l, r) for l, r in cases.values()))
    assert len(lines) == 9 * len(cases)
    for j, (name, (left, right)) in enumerate(cases.items()):
        levels, s = parse_shape(lines[9 * j:9 * j + 9])
        check(left, right, levels, s)
    assert len(parse_shape(lines[9 * (len(cases) - 1):])[1]["roots"]) == 3  # forest3 is the last one


def test_chain_of_2_to_the_20(run):
    n = 1 << 20
    assert run(f"chain {n} 0\nchain {n} 1") == [f"chain {n} 1 {n - 1} {n - 1} 0", f"chain {n} 1 {n - 1} 0 {n - 1}"]


def test_malformed_children_are_refused(run):
    lines = run("\n".join(tree_line(l, r) for _, l, r in TC.REFUSED))
    assert len(lines) == len(TC.REFUSED)
    want = {"child_is_n": "child index", "child_minus_2": "child index", "self_child": "own child", "two_parents": "two parents",
            "left_equals_right": "two parents", "cycle_alone": "cycle", "cycle_beside_a_tree": "cycle"}
    for (name, _, _), ln in zip(TC.REFUSED, lines):
        assert ln.startswith("refused # ") and want[name] in ln, (name, ln)
