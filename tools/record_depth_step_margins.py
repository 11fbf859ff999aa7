"""
tests/golden/depth_step_margins.json from several MI355X runs of tests/test_gpu_depth_step.py.

    rm tests/golden/depth_step_margins.json; pytest tests/test_gpu_depth_step.py -m gpu; cp tests/golden/depth_step_margins.json run1.json
    ... (again for run2.json, run3.json)
    python tools/record_depth_step_margins.py run1.json run2.json run3.json

Each run writes the file through test_gpu_train_step.settle when it is absent; this keeps, per row, the LARGEST of the runs' values
and says so in the note.  One run is not enough for the rows paths/D6 and paths/D7: they compare two float32 runs that differ by
the order of their float atomics alone, and two runs of the same tree gave 9.9e-6 and 1.2e-4 for paths/D6/rotations, more than the
factor 10 a later run is allowed over the record.
"""
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "depth_step_margins.json")


def main(paths):
    docs = [json.load(open(p)) for p in paths]
    keys = set(docs[0]["worst"])
    assert all(set(d["worst"]) == keys for d in docs), "the runs disagree on the rows"
    note = docs[0]["_note"] + f"; each value is the largest of {len(docs)} runs (tools/record_depth_step_margins.py)"
    doc = {"_note": note, "worst": {k: max(d["worst"][k] for d in docs) for k in sorted(keys)}}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"{OUT}: {len(keys)} rows, largest {max(doc['worst'].values()):.3g}")


if __name__ == "__main__":
    main(sys.argv[1:])
