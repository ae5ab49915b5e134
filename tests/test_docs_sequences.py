"""The numbers README.md and DESIGN.md quote for the sequence entries are the lines of profiles/r18/sequences.json (tools/bench_sequences.py), and those lines
are of the committed sources: same build stamp as the library's."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_documents_quote_the_committed_sequence_lines(zj):
    with open(os.path.join(ROOT, "profiles", "r18", "sequences.json")) as f:
        lines = [json.loads(x) for x in f.read().strip().splitlines()]
    assert [x["shape"] for x in lines] == ["metric_65536x65536", "large_1024x1048576"]
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())          # (the paragraphs are wrapped: a figure may sit on both sides of a line end)
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    for x in lines:
        assert x["build_stamp"] == zj.build_stamp(), "the lines are of another build than the committed sources"
        assert x["steps"] >= 5 and x["warmup"] >= 1 and "repeated" in x["replicated"]
        quoted = "**%.3f ms = %.1f GiB/s**" % (x["sequences_ms"], x["sequences_GiBps"])
        plain = "%.3f ms = %.2f GiB/s" % (x["plain_ms"], x["plain_GiBps"])
        for name, text in (("DESIGN.md", design), ("README.md", readme)):
            assert quoted in text and plain in text, (name, quoted, plain)
    assert "%.3f ms" % lines[0]["plain_match_ms"] in design and lines[0]["build_stamp"] in design
    assert "replicated" in design and "replicated" in readme
