"""tree_shape_touched of csrc/tree_shape.h -- the touched nodes and all their ancestors, grouped by height -- compiled for the host
under -fsanitize=address,undefined (tools/hosttest/tree_touched_test.cpp, a stand-alone program) and held against the plain parent
walk of tests/tree_touched_cases.py over the shapes of tests/tree_cases.py: empty lists, every single node of the shapes of at most
70 nodes, random subsets, lists with duplicates, all nodes; a left chain of 2^20 nodes with its deepest node touched (2^20 levels:
the case that catches recursion); and an index equal to n, refused with a message that names it. Exit status 0 and an empty stderr
throughout."""
import subprocess

import pytest

import hosttest
import tree_cases as TC
import tree_touched_cases as TT


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = hosttest.build(tmp_path_factory.mktemp("tree_touched"), "tree_touched_test",
                         flags=("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), mp2g_h=False)

    def go(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stdout[-300:] + r.stderr[-2000:]
        return r.stdout.splitlines()
    return go


def tree_line(left, right):
    return f"tree {len(left)} " + " ".join(f"{l} {r}" for l, r in zip(left, right))


def numbers(line, name):
    t = line.split()
    assert t[0] == name, line
    return [int(x) for x in t[1:]]


def test_closures_of_the_accepted_shapes(run):
    cases = TC.accepted(small=False)
    text, sets = [], {}
    for j, (name, (left, right)) in enumerate(cases.items()):
        sets[name] = TT.touched_sets(len(left), 0x70C + j)
        text.append(tree_line(left, right))
        text += [f"touch {len(t)} " + " ".join(map(str, t)) for _, t in sets[name]]
    lines = iter(run("\n".join(text)))
    for name, (left, right) in cases.items():
        assert next(lines).startswith("ok "), name
        assert numbers(next(lines), "parent") == TT.parents(left, right), name
        for what, t in sets[name]:
            nodes, off = TT.closure(left, right, t)
            assert numbers(next(lines), "nodes") == nodes, (name, what)
            assert numbers(next(lines), "off") == off, (name, what)
    assert next(lines, None) is None


def test_chain_of_2_to_the_20_touched_at_its_deepest_node(run):
    n = 1 << 20
    assert run(f"deep {n}") == [f"deep {n} {n} 1 {n - 1} 0 {n * (n - 1) // 2}"]


def test_an_index_outside_the_shape_is_refused_and_leaves_no_mark(run):
    left, right = TC.sbbst(7)
    lines = run("\n".join([tree_line(left, right), "touch 1 7", "touch 3 0 4 7", "touch 1 4294967295", "touch 2 0 4", "touch 0",
                           "tree 0 ", "touch 1 0", "touch 0"]))
    assert lines[0] == "ok 3"
    for ln, bad in zip(lines[2:5], ("7", "7", "4294967295")):
        assert ln.startswith("refused # ") and f"index {bad} " in ln, ln
    nodes, off = TT.closure(left, right, [0, 4])  # the nodes marked before the refusal of "0 4 7" were cleared again
    assert numbers(lines[5], "nodes") == nodes and numbers(lines[6], "off") == off
    assert lines[7:9] == ["nodes", "off 0"]
    assert lines[9:11] == ["ok 0", "parent"]
    assert lines[11].startswith("refused # ") and "index 0 " in lines[11]
    assert lines[12:] == ["nodes", "off 0"]
