"""tools/exp_http.py builds kernel variants by text substitution on csrc/
sources.  A substitution whose old text has left the sources otherwise fails
only when somebody builds that variant on a GPU box; this checks every one."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "cilium_amd" / "csrc"


def test_every_variant_anchor_is_in_its_source():
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        from exp_http import VARIANTS
    finally:
        sys.path.remove(str(ROOT / "tools"))
    assert "base" in VARIANTS
    checked, stale = 0, []
    for name, subs in VARIANTS.items():
        for sub in subs:
            fn, old, _new = sub if len(sub) == 3 else ("kernels_http.hip", *sub)
            src = CSRC / fn
            checked += 1
            if not src.is_file():
                stale.append(f"{name}: no csrc/{fn}")
            elif old not in src.read_text():
                stale.append(f"{name}: not in csrc/{fn}: {old!r}")
    assert checked > 50  # the substitutions were read, not an empty table
    assert not stale, "\n".join(stale)
