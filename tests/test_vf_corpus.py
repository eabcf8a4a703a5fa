"""The graph layer of profile.py against the record of the tree before it was rewritten
(tests/golden/vf_corpus_digests.json, written by tests/vf_corpus.py from that tree): every graph of
the two corpora parses to the same Profile or is refused with the same reason, letter for letter.
And the one change made on purpose: of several -vf options the last one wins."""
import json
import os

import pytest

import vf_corpus
from ffmpeg_distributed_amd import profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vf_corpus_digests.json")
TAIL = vf_corpus.TAIL

HOW_TO_DIFF = """
To see the graphs that differ, list both trees and diff the listings (about 16 MB each):
    git worktree add /tmp/vf_parent <the commit the golden file was written from>
    python tests/vf_corpus.py --root /tmp/vf_parent --list /tmp/vf_a
    python tests/vf_corpus.py --list /tmp/vf_b
    diff /tmp/vf_a/{name}.txt /tmp/vf_b/{name}.txt | head
(tools/README.md, "The -vf corpus")."""


@pytest.mark.parametrize("name", sorted(vf_corpus.CORPORA))
def test_every_graph_of_the_corpus_parses_as_before(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = vf_corpus.digests(vf_corpus.load_profile(), name)
    assert sorted(got) == sorted(want), "the corpus itself changed: its first filters differ"
    differ = [first for first in want if got[first] != want[first]]
    assert not differ, (f"{name}: graphs that start with {differ} parse differently: "
                        + "; ".join(f"{k}: {got[k]['graphs']} graphs, {got[k]['accepted']} accepted (were "
                                    f"{want[k]['graphs']}, {want[k]['accepted']})" for k in differ)
                        + HOW_TO_DIFF.format(name=name))


def test_the_corpora_are_what_the_golden_file_counts():
    # 18 tokens: 18 + 18^2 + 18^3 + 18^4 sequences; the accepted ones are few, and none holds a ';'
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sum(b["graphs"] for b in want["corpus1"].values()) == 18 + 18 ** 2 + 18 ** 3 + 18 ** 4
    assert want["corpus1"]["null;null"]["accepted"] == 0 and want["corpus2"]["null;null"]["accepted"] == 0
    assert sum(b["accepted"] for b in want["corpus1"].values()) == 662
    assert sum(b["accepted"] for b in want["corpus2"].values()) == 3134


EARLIER = "yadif,vflip,crop=32:16,scale=64:32,unsharp,pad=80:48"


@pytest.mark.parametrize("a,b", [
    (EARLIER, "eq=1.2"),
    (EARLIER, "colormatrix=bt709:bt601"),
    (EARLIER, "colormatrix=bt709:bt601,eq=1.2"),
    (EARLIER, "scale=64:32"),
    ("eq=1.2", "scale=64:32"),
    ("colormatrix=bt709:bt601,eq=1.2", "vflip"),
])
def test_the_last_vf_replaces_every_chain_field_of_an_earlier_one(a, b):
    alone = profile.parse(f"-vf {b}{TAIL}")
    assert profile.parse(f"-vf {a} -vf {b}{TAIL}") == alone
    assert profile.parse(f"-filter:v {a}{TAIL} -vf {b}") == alone
    assert profile.parse(f"-vf {a}{TAIL}") != alone          # the earlier graph alone is another profile


def test_a_refused_vf_is_refused_wherever_it_stands():
    alone = profile.try_parse(f"-vf hue=s=0{TAIL}")
    assert alone == (None, "filter graph 'hue=s=0' (only crop, scale or crop,scale is GPU-accelerated)")
    assert profile.try_parse(f"-vf hue=s=0 -vf eq=1.2{TAIL}") == alone       # parsing stays eager
    assert profile.try_parse(f"-vf eq=1.2 -vf hue=s=0{TAIL}") == alone


def test_a_graph_with_a_semicolon_is_refused_whatever_it_names():
    for vf in ("null;null", "yadif;eq=1.2", "colormatrix=bt709:bt601,scale=64:32;null"):
        assert profile.try_parse(f"-vf {vf}{TAIL}") == (
            None, f"filter graph {vf!r} (only crop, scale or crop,scale is GPU-accelerated)")


def test_parse_graph_names_only_the_fields_the_graph_sets():
    assert profile.parse_graph("vflip") == {"orient": 4}
    assert profile.parse_graph("vflip,vflip") == {"orient": 0}
    assert profile.parse_graph("yadif,scale=64:32,eq=1.2") == {
        "deint": {"mode": 0, "parity": -1}, "scale": (64, 32), "sws_flags": ("bicubic",),
        "eq": dict(profile.EQ_DEFAULT, contrast=1.2, slot="out")}
    assert set(profile.parse_graph("colormatrix=bt709:bt601,crop=32:16,unsharp,pad=80:48")) == {
        "colormatrix", "crop", "unsharp", "pad"}
