"""csrc/layout.h compiled for the host (tools/hosttest/layout_test.cpp): for the proof shapes of test_verifier_host.SHAPES and the
edge shapes of tests/golden/fri_layout_parent.json (no layers, no queries, one oracle, a layer without siblings, mixed arities with
lookup polynomials, the Z polynomials outside oracle 2) the sections of the flat FRI proof are contiguous and in the documented order,
the opening offsets enumerate the openings once and agree with fri_batch_poly, and the sizes are the ones the library returned
BEFORE the layout had one definition -- recorded in the golden file from that build, not recomputed here."""
import json
import os
import subprocess

import pytest

import circuits as C
import hosttest
import oracle as O
from test_verifier_host import SHAPES

GOLDEN = json.load(open(os.path.join(O.ROOT, "tests", "golden", "fri_layout_parent.json")))["cases"]
FIELDS = ["variant", "log_n", "rate_bits", "cap_height", "pow_bits", "num_queries", "n_layers", "arity_bits", "n_oracles", "oracle_w",
          "zs_oracle", "zs_count", "num_lookup_polys"]


@pytest.fixture(scope="module")
def layout_test(tmp_path_factory):
    return hosttest.build(tmp_path_factory.mktemp("layout"), "layout_test")


def words(params):
    out = []
    for f in FIELDS:
        v = params[f]
        out += [int(x) for x in v] if isinstance(v, list) else [int(v)]
    assert len(out) == 27
    return out


def test_golden_covers_the_required_shapes(mp2):
    """the first cases of the golden file ARE the verifier's test shapes (built here from SHAPES), the rest the edge cases"""
    for (log_n, kinds, lookups), case in zip(SHAPES, GOLDEN):
        sel = {"ALL_KINDS": 6, "LEAF_KINDS": 5, "VERIFIER_KINDS": 4}[kinds]
        nlp = C.NUM_LOOKUP_POLYS if lookups else 0
        fp = mp2.standard_recursion_params(log_n, (sel + (6 if lookups else 0) + 2 + 80, 135, 2 * (10 + nlp), 16), num_lookup_polys=nlp)
        got = {f: (list(getattr(fp, f)) if f in ("arity_bits", "oracle_w") else int(getattr(fp, f))) for f in FIELDS}
        assert got == case["params"], case["name"]
    by = {c["name"]: c["params"] for c in GOLDEN}
    assert len(GOLDEN) >= len(SHAPES) + 4
    assert by["no_layers"]["n_layers"] == 0 and by["no_queries"]["num_queries"] == 0 and by["one_oracle"]["n_oracles"] == 1
    p = by["layer_without_siblings"]
    assert p["log_n"] + p["rate_bits"] - p["arity_bits"][0] == p["cap_height"]


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_layout(layout_test, case):
    for n_pi in (0, 4, 9):
        r = subprocess.run([layout_test, str(case["num_constants"]), str(n_pi)] + [str(w) for w in words(case["params"])], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.split() == ["proof_words", str(case["proof_words"]), "n_open", str(case["n_openings"]), "bad", "0"], r.stdout + r.stderr


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_exported_sizes(mp2, case):
    """mp2g_fri_proof_words / mp2g_fri_n_openings still return what they returned"""
    fp = mp2.FriParams()
    for f in FIELDS:
        v = case["params"][f]
        if isinstance(v, list):
            for i, x in enumerate(v):
                getattr(fp, f)[i] = x
        else:
            setattr(fp, f, v)
    assert fp.proof_words == case["proof_words"] and fp.n_openings == case["n_openings"]
