"""Record tests/golden/plan_trace.json: for every case of tests/plan_trace.py, with ``use_graph`` off and on, the engine calls a
recording stand-in saw, the keys of every step's rows and the error that ended the case, if one did -- packed (plan_trace.pack):
the traces repeat themselves from step to step and from case to case.  Run it on the commit whose behaviour is to be pinned:  python tests/golden/make_plan_trace.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
from plan_trace import pack, record_all, unpack  # noqa: E402


def dump(packed):
    """One table entry, segment, report or case per line: a change of a trace reads as a diff of a few lines."""
    def lines(items):
        return "[\n" + ",\n".join("  " + json.dumps(item) for item in items) + "]"

    def table(name):
        return "{\n" + ",\n".join(f"  {json.dumps(key)}: {json.dumps(value)}" for key, value in packed[name].items()) + "}"
    return (f'{{"calls": {lines(packed["calls"])},\n"keys": {lines(packed["keys"])},\n"reports": {table("reports")},\n'
            f'"segments": {table("segments")},\n"cases": {table("cases")}}}\n')


if __name__ == "__main__":
    record = record_all()
    text = dump(pack(record))
    assert all(unpack(json.loads(text), name) == case for name, case in record.items())
    with open(os.path.join(HERE, "plan_trace.json"), "w") as out:
        out.write(text)
    print(f"{len(text)} bytes")
