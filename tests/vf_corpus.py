"""Two generated corpora of `-vf` graphs and what profile.try_parse makes of each: the record that
a change to the graph layer of profile.py is compared against, graph for graph and letter for letter.

    python tests/vf_corpus.py                      digests of this tree, as JSON on stdout
    python tests/vf_corpus.py --list DIR           DIR/corpus1.txt, DIR/corpus2.txt: `graph<TAB>outcome` lines
    python tests/vf_corpus.py --root OTHER_TREE    the same with OTHER_TREE's profile.py (a worktree of
                                                   another commit), for `diff` against this tree's listing

The outcome is the Profile as sorted JSON, or "! " and the reason of a refused graph.  The wall time
goes to stderr.  tests/golden/vf_corpus_digests.json holds, per corpus and per first filter of the
graph, the number of graphs, the number accepted and the SHA-256 of those lines in generation order;
it was written by this script from the tree before the graph layer was rewritten (tools/README.md).
Nothing of the package but `profile` is imported, so any tree that has a profile.py can be listed."""
import argparse
import dataclasses
import hashlib
import importlib.util
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = " -c:v mjpeg -q:v 5 -dct int -bitexact"
TOKENS = ("yadif", "yadif=2:bff", "bwdif", "vflip", "transpose=1", "hflip", "colormatrix=bt709:bt601", "eq=1.2",
          "crop=32:16:2:2", "crop", "scale=64:32", "unsharp", "pad=80:48", "pad", "hue=s=0", "eq=", "colormatrix=bt709",
          "null;null")
CHAIN = ("yadif", "vflip", "transpose=1", "colormatrix=bt709:bt601", "eq=1.2", "crop=32:16:2:2", "scale=64:32",
         "eq=gamma=1.1", "unsharp", "pad=80:48")


def load_profile(root=ROOT):
    """profile.py of the tree at `root`, loaded by path (no other module of the package runs)."""
    path = os.path.join(root, "ffmpeg_distributed_amd", "profile.py")
    spec = importlib.util.spec_from_file_location("_vf_corpus_profile", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod           # dataclasses looks the module up while the class is made
    spec.loader.exec_module(mod)
    return mod


def corpus1():
    """Every sequence of 1 to 4 tokens."""
    for n in range(1, 5):
        for seq in itertools.product(TOKENS, repeat=n):
            yield seq


def corpus2():
    """Every non-empty subset of the canonical chain in chain order: itself, with each one adjacent
    pair swapped, and with each one token inserted at each position; a graph that comes up again
    (a chain token inserted where the next subset has it) is listed once, where it came up first."""
    seen = set()

    def variants(sub):
        yield sub
        for i in range(len(sub) - 1):
            yield sub[:i] + (sub[i + 1], sub[i]) + sub[i + 2:]
        for t in TOKENS:
            for i in range(len(sub) + 1):
                yield sub[:i] + (t,) + sub[i:]

    for mask in range(1, 1 << len(CHAIN)):
        for seq in variants(tuple(t for i, t in enumerate(CHAIN) if mask >> i & 1)):
            if seq not in seen:
                seen.add(seq)
                yield seq


CORPORA = {"corpus1": corpus1, "corpus2": corpus2}


def outcome(profile, graph):
    prof, why = profile.try_parse("-vf " + graph + TAIL)
    if prof is None:
        return "! " + why
    return json.dumps(dataclasses.asdict(prof), sort_keys=True)


def lines(profile, name):
    """(first filter, accepted, `graph<TAB>outcome\\n`) for every graph of a corpus, in generation order."""
    for seq in CORPORA[name]():
        graph = ",".join(seq)
        out = outcome(profile, graph)
        yield seq[0], not out.startswith("! "), f"{graph}\t{out}\n"


def digests(profile, name):
    """{first filter: {"graphs", "accepted", "sha256"}} of one corpus."""
    acc = {}
    for first, ok, line in lines(profile, name):
        b = acc.setdefault(first, [0, 0, hashlib.sha256()])
        b[0] += 1
        b[1] += ok
        b[2].update(line.encode())
    return {k: {"graphs": n, "accepted": a, "sha256": h.hexdigest()} for k, (n, a, h) in acc.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=ROOT, help="the tree whose ffmpeg_distributed_amd/profile.py is listed")
    ap.add_argument("--list", metavar="DIR", help="write the full listings into DIR instead of the digests")
    a = ap.parse_args(argv)
    profile = load_profile(a.root)
    t0 = time.perf_counter()
    if a.list:
        os.makedirs(a.list, exist_ok=True)
        for name in CORPORA:
            with open(os.path.join(a.list, name + ".txt"), "w") as f:
                f.writelines(line for _, _, line in lines(profile, name))
    else:
        json.dump({name: digests(profile, name) for name in CORPORA}, sys.stdout, indent=1, sort_keys=True)
        sys.stdout.write("\n")
    sys.stderr.write(f"vf_corpus: {time.perf_counter() - t0:.2f} s\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
