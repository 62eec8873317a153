"""Stand-in for ``pygtrie`` (see kenlm.py in this directory): the two calls KenlmScorer makes on a CharTrie."""


class CharTrie:
    def __init__(self):
        self._nodes = set()

    @classmethod
    def fromkeys(cls, keys, value=None):
        trie = cls()
        for key in keys:
            trie._nodes.update(key[:k] for k in range(len(key) + 1))
        return trie

    def has_node(self, key):
        return key in self._nodes
