"""The forms of the CIGAR text as a Python model written from the rules of include/scrooge_amd.h (CIGAR FORMS).  Nothing here
calls the library.

The class of a run is its operation under "merged"; under "m", '=' and 'X' have class 'M' and 'I' and 'D' keep theirs.  The text
of a pair is, for every maximal stretch of directly adjacent runs of one class, the decimal sum of their counts and the class
letter.  "windowed" prints every run by itself.  A pair without runs has ""."""
import itertools
import re

FORMS = ["merged", "m"]

# runs as the windows leave them -> merged, m
TABLE = [
    ("29=21=", "50=", "50M"),
    ("31I13I16=2I2I", "44I16=4I", "44I16M4I"),
    ("4=1X2=1D2=", "4=1X2=1D2=", "7M1D2M"),
    ("", "", ""),
]


def parse(cigar):
    """"29=21=" -> [(29, "="), (21, "=")]"""
    runs = [(int(n), o) for n, o in re.findall(r"(\d+)([=XID])", cigar)]
    assert "".join("%d%s" % r for r in runs) == cigar, "not a windowed CIGAR: %r" % cigar[:40]
    return runs


def model(form, runs):
    """The text of one pair's runs [(count, op)] in a form: "windowed", "merged" or "m"."""
    if form == "windowed":
        return "".join("%d%s" % r for r in runs)
    assert form in FORMS
    cls = (lambda o: "M" if o in "=X" else o) if form == "m" else (lambda o: o)
    return "".join("%d%s" % (sum(n for n, _ in g), c) for c, g in itertools.groupby(runs, key=lambda r: cls(r[1])))


def stretches(text):
    """"50=4I" -> [(50, "="), (4, "I")]; asserts that the text is nothing but such items"""
    items = [(int(n), o) for n, o in re.findall(r"(\d+)([=XIDM])", text)]
    assert "".join("%d%s" % i for i in items) == text, "malformed CIGAR %r" % text[:40]
    return items
