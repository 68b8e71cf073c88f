"""Park, swap, undo: how every ``patch_reference_*`` puts a dispatcher in the place of one of the reference's own names.  The
original is parked next to it as ``_reference_<name>``, once; the swap is the caller's; the undo binds the original back.
``patch_forwards`` / ``unpatch_forwards`` are that rule for the ``forward`` of a list of classes in a list of modules, and
``run_reference`` is how a dispatcher reaches the parked original again."""
import importlib
import sys


def park(owner, name):
    """Store ``owner.<name>`` (``owner``: a module or a class) as ``owner._reference_<name>`` unless ``owner`` itself holds one
    already -- a subclass that inherits a parked attribute parks its own -- and return the parked original."""
    if "_reference_" + name not in vars(owner):
        setattr(owner, "_reference_" + name, getattr(owner, name))
    return getattr(owner, "_reference_" + name)


def unpark(owner, name):
    """Bind the parked original back as ``owner.<name>`` and drop the parked attribute; nothing when it was never parked."""
    if "_reference_" + name in vars(owner):
        setattr(owner, name, getattr(owner, "_reference_" + name))
        delattr(owner, "_reference_" + name)


def patch_forwards(modules, classes):
    """Bind ``fwd`` as ``cls.forward`` for every ``(class name, fwd)`` of ``classes`` that each of ``modules`` (names to import, or
    module objects) holds, the original parked.  A name that does not import is skipped (a reference module whose own imports
    are missing here: nothing to patch), and so is a class that is not there.  Idempotent: only a ``forward`` that is still the
    parked original is replaced.  Returns the module objects it went through."""
    done = []
    for mod in modules:
        if isinstance(mod, str):
            try:
                mod = importlib.import_module(mod)
            except Exception:                            # noqa: BLE001
                continue
        for cls_name, fwd in classes:
            cls = getattr(mod, cls_name, None)
            if cls is not None and cls.forward is park(cls, "forward"):
                cls.forward = fwd
        done.append(mod)
    return done


def unpatch_forwards(modules, class_names):
    """Undo ``patch_forwards``: ``unpark`` the ``forward`` of every class of ``class_names`` that each of ``modules`` holds; a name
    is looked up in ``sys.modules`` (never imported), a module object is taken as it is."""
    for mod in modules:
        mod = sys.modules.get(mod) if isinstance(mod, str) else mod
        for cls_name in class_names:
            if hasattr(mod, cls_name):
                unpark(getattr(mod, cls_name), "forward")


def run_reference(obj, fallback, *args, **kw):
    """What a dispatcher hands a call that the kernels do not take: the parked ``_reference_forward`` of ``obj``'s type, called
    as the method it was; where nothing is parked (a stand-in class of the tests and tools) ``fallback(*args, **kw)``;
    AttributeError without either."""
    ref = getattr(type(obj), "_reference_forward", None)
    if ref is not None:
        return ref(obj, *args, **kw)
    if fallback is None:
        raise AttributeError("%s has no parked _reference_forward and its dispatcher names no fallback" % type(obj).__name__)
    return fallback(*args, **kw)


def rebind_everywhere(mapping, skip=()):
    """Every module that bound one of ``mapping``'s keys by name (``from ddsp.core import upsample`` in flask_api.py:12,
    gui_diff.py:10, main_reflow.py:13, ...; ``from ddsp.vocoder import CombSubFast`` in diffusion/vocoder.py:13) gets the value
    instead -- found by IDENTITY over ``sys.modules``, so no list of importers has to be kept up to date.  Attributes whose name
    starts with ``_reference_`` (where the originals are parked) and the modules in ``skip`` are left alone.  Returns the
    bindings it changed as ``(module, name, old value, new value)`` -- ``undo_rebound`` undoes exactly those."""
    ids = {id(k): v for k, v in mapping.items()}
    changed = []
    for mod in list(sys.modules.values()):
        if mod is None or mod in skip:
            continue
        try:
            items = list(vars(mod).items())
        except TypeError:                                # a module-like object without a __dict__
            continue
        for name, val in items:
            new = ids.get(id(val))
            if new is not None and not name.startswith("_reference_"):
                try:
                    setattr(mod, name, new)
                    changed.append((mod, name, val, new))
                except Exception:                        # noqa: BLE001  (read-only module objects)
                    pass
    return changed


def undo_rebound(changed):
    """Empty ``changed`` (what ``rebind_everywhere`` returned): each binding goes back to its old value where it is still the
    new one; a binding that somebody else changed since is left as it is."""
    while changed:
        mod, name, old, new = changed.pop()
        if getattr(mod, name, None) is new:
            setattr(mod, name, old)
