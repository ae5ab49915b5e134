"""The numbers README.md and DESIGN.md quote for the generate entries are the lines of profiles/r19/generate.json (tools/bench_generate.py), and those lines
are of the committed sources: same build stamp as the library's."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_documents_quote_the_committed_generate_lines(zj):
    with open(os.path.join(ROOT, "profiles", "r19", "generate.json")) as f:
        lines = [json.loads(x) for x in f.read().strip().splitlines()]
    assert [(x["shape"], x["level"]) for x in lines] == [("metric_65536x65536", 3), ("metric_65536x65536", 1), ("large_1024x1048576", 3)]
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())          # (the paragraphs are wrapped: a figure may sit on both sides of a line end)
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    for x in lines:
        assert x["build_stamp"] == zj.build_stamp(), "the lines are of another build than the committed sources"
        assert x["steps"] >= 5 and x["warmup"] >= 1 and x["route"] == "wave" and x["frames_compared_with_reference"] >= 8
        quoted = "**%.3f ms = %.1f GiB/s**" % (x["generate_ms"], x["generate_GiBps"])
        plain = "%.3f ms = %.2f GiB/s" % (x["plain_ms"], x["plain_GiBps"])
        assert quoted in design and plain in design, (quoted, plain)
    assert "**%.3f ms = %.1f GiB/s**" % (lines[0]["generate_ms"], lines[0]["generate_GiBps"]) in readme
    assert lines[0]["build_stamp"] in design
