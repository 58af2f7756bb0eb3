"""Write tests/golden/workspace_layout.json: the answers of the built library to the table of
tests/ws_layout_cases.py (workspace sizes, layouts, status offsets and host-side refusal codes).

    python tools/record_workspace_layout.py

Run it on the commit whose layout is to be kept, BEFORE changing csrc/: the file pins every byte
offset callers and tools rely on, and tests/test_host_workspace_layout.py holds later builds to it.
Needs no GPU.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('iou-aware-single-stage-object-detector_amd', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))

if __name__ == '__main__':
    import ws_layout_cases
    from iouaware import _lib
    rec = ws_layout_cases.record(_lib.lib())
    out = os.path.join(ROOT, 'tests', 'golden', 'workspace_layout.json')
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write('\n')
    print('%s: %d layout answers, %d refusals' % (out, len(rec['layout']), len(rec['refusal'])))
