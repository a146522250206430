"""What the tests/test_*_abi.py files share: include/wifirx.h as text, and the argument list of a declaration in it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_raw():
    return open(os.path.join(ROOT, "include", "wifirx.h")).read()


def _header():
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", "", _header_raw(), flags=re.S)


def _decl(txt, name):
    """the text between the parentheses of `name`'s declaration"""
    return re.search(r"\b%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S).group(1)


def _norm(decl):
    """its arguments, white space normalised"""
    return [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")]
