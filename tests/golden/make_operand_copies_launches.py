"""Writes tests/golden/operand_copies_launches.json: per scenario of tests/test_operand_copies_cpu.py (training steps over the switches, the
input-gradient and frozen-prefix steps, forward_views on two resolutions, every inspection call inside a training step) the names of the launches
and a SHA-256 over each launch's name, argument shapes, dtypes, strides and keyword arguments.  No GPU and no kernel: the test's recorder stands
in for every hip.* wrapper.

    python tests/golden/make_operand_copies_launches.py

The committed record was made on the commit BEFORE the operand copies became a value (the scenarios use public calls only, so the test module
runs there unchanged): the test holds every later commit to that commit's launches.  Run it again only where a change of the launch sequences is
the purpose of the commit."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_operand_copies_cpu as t  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    rec = t.record_all()
    with open(out, "w") as fh:
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rec.items()) + "\n}\n")
    print(f"wrote {out}: {len(rec)} scenarios, {sum(len(v['names']) for v in rec.values())} launches")
