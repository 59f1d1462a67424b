"""Behaviour A/B of the batch round trip between two builds of librsn (RSN_LIB_PATH names the other one): what the one-list call launches,
copies and answers, printed so that two builds' outputs can be compared line for line -- no time, no date, no address.

    timeout -k 10 300 python scripts/probes/roundtrip_one_flow_ab.py [out_file]     (default: standard output only)

A line a case: the return code, the message, a digest of the rows and histograms, the bytes on copy commands up and down, and the full
launch profile (every name and count).  The cases are tests/test_gpu_roundtrip_batch.py's, through its own raw callers: [lzss, huffman]
over the 64 members of 8 to 12 KiB in both forms with and without histograms, [lzss, huffman, lzss] over 6 members a run each, no layers,
and an empty member failing in the Huffman layer in one run and a run a member.  One suite call with a kept node stands at the end."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from raisin_amd import _lib  # noqa: E402
from test_gpu_batch_dev import _prof  # noqa: E402
from test_gpu_roundtrip_batch import GROUPED, HU, LZ, MEMBERS, _dev, _host, _text  # noqa: E402
from test_gpu_suite_batch import _suite  # noqa: E402


def main():
    _lib.check(_lib.lib().rsn_device_set(0))
    lines = []

    def case(name, call, budget=None):
        if budget:
            os.environ["RSN_LAYERS_BATCH_BUDGET"] = budget
        try:
            got, prof, (up, down) = _prof(_lib, call)
        finally:
            os.environ.pop("RSN_LAYERS_BATCH_BUDGET", None)
        rc, msg = got[0], got[-1] if got[0] else ""
        digest = hashlib.sha256(repr(got[1:-1]).encode()).hexdigest()[:16]
        line = "%-44s rc %d  answers %s  up %d down %d  %s  %s" % (name, rc, digest, up, down, " ".join("%s=%d" % kv for kv in sorted(prof.items())), msg)
        print(line.rstrip(), flush=True)
        lines.append(line.rstrip())
    for form in (_host, _dev):
        for hists in (True, False):
            case("[lzss, huffman] 64 x 8-12 KiB %s hists=%d" % (form.__name__, hists), lambda: form(_lib, GROUPED, [LZ, HU], hists))
    datas = MEMBERS[:8] + MEMBERS[9:]
    for form in (_host, _dev):
        case("[lzss, huffman, lzss] 6 members budget 1 %s" % form.__name__, lambda: form(_lib, datas[:6], [LZ, HU, LZ]), budget="1")
        case("no layers %s" % form.__name__, lambda: form(_lib, MEMBERS, []))
    failing = [_text(1, 500), _text(2, 900), b"", _text(3, 700), b""]
    for budget in (None, "1"):
        for form in (_host, _dev):
            case("empty member [lzss, huffman] budget %s %s" % (budget, form.__name__), lambda: form(_lib, failing, [LZ, HU]), budget)
            case("empty member [huffman, lzss] budget %s %s" % (budget, form.__name__), lambda: form(_lib, failing, [HU, LZ], False), budget)
    for form in ("host", "dev"):
        case("suite {[lzss], [lzss, huffman], [huffman]} %s" % form, lambda: _suite(_lib, form, failing[:2] + MEMBERS[:8], [[LZ], [LZ, HU], [HU]]))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
