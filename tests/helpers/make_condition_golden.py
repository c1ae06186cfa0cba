"""Records tests/golden/conditions_match.json: a small annotation / results pair (condition_cases.golden_input) and the
cond_kpts the reference's matching script produces for it.

    python tests/helpers/make_condition_golden.py <reference root>

The script (data_preprocessing/match_coco_cond.py) is read at run time: its function definitions and the loop over the
annotations inside its __main__ block are compiled from its own syntax tree and run on the pair.  Its imports are not
executed - it imports pycocotools and never uses it - and its file names, which are placeholders, are not read.  Only
the data is written."""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "conditions_match.json")


def _plain(obj):
    if isinstance(obj, np.integer):
        return int(obj)
    if isinstance(obj, np.floating):
        return float(obj)
    raise TypeError(type(obj))


def run_script_loop(script, gt_annotations, pred_results, model):
    tree = ast.parse(open(script).read())
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef)]
    main = [n for n in tree.body if isinstance(n, ast.If)][-1]
    loops = [n for n in ast.walk(main) if isinstance(n, ast.For) and isinstance(n.iter, ast.Subscript)
             and getattr(n.iter.value, "id", None) == "gt_annotations"]
    assert len(loops) == 1, "the loop over gt_annotations['annotations'] was not found"
    scope = {"np": np, "gt_annotations": gt_annotations, "pred_results": pred_results, "model": model}
    exec(compile(ast.Module(body=defs + loops, type_ignores=[]), script, "exec"), scope)
    return gt_annotations


def main(reference_root):
    from tests.helpers import condition_cases as cases
    gt, results = cases.golden_input()
    annotated = run_script_loop(os.path.join(reference_root, "data_preprocessing", "match_coco_cond.py"),
                                json.loads(json.dumps(gt)), results, cases.MODEL_KEY)
    cond = {str(a["id"]): a["cond_kpts"][cases.MODEL_KEY] for a in annotated["annotations"]}
    with open(OUT, "w") as f:
        json.dump({"gt": gt, "results": results, "model": cases.MODEL_KEY, "cond_kpts": cond}, f, default=_plain)
    print(f"wrote {OUT}: {len(cond)} annotations, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
