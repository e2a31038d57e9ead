// twilight_amd/csrc/host/partition.cpp -- the guide tree cut into subtrees of at most N leaves (-m / --max-subtree).
// Behavioural mirror of the reference's src/partitionInfo.cpp:7-110 (called with minPartitionSize = 0), phylogeny.cpp:13-39 and
// tree.cpp:519-526; every routine cites the lines it follows.  Pure host code on phylogeny::Node: tests/partition_kats.cpp links it
// with phylo.cpp alone.
//
// What is observable of the reference's search: a subtree is split at the internal node whose number of leaves (inside the subtree) is
// closest to half of the subtree's; of several equally close ones the first in post-order (children left to right, then the node) wins; a
// leaf is never a split point; a subtree whose best split point is its own root stays as it is, however large.  The split-off part gets
// the next free index, the rest keeps its own.  The reference walks the tree recursively and counts the leaves below every candidate
// again; here one walk counts them all and the search is iterative (a caterpillar of 100 000 leaves is as deep as it is large).
#include "twl_host.hpp"

#include <algorithm>

namespace phylogeny {

namespace {

// the nodes of root's group below root (root included) in pre-order, children left to right
void groupPreOrder(Node *root, std::vector<Node *> &out)
{
    out.clear();
    const int grp = root->grpID;
    std::vector<Node *> work{root};
    while (!work.empty()) {
        Node *cur = work.back();
        work.pop_back();
        out.push_back(cur);
        for (int i = (int)cur->children.size() - 1; i >= 0; --i)
            if (cur->children[i]->grpID == grp) work.push_back(cur->children[i]);
    }
}

// getNumLeaves (partitionInfo.cpp:7-14) of every node of root's group at once: schedIdx is the node's slot in `order`
void leavesBelow(Node *root, std::vector<Node *> &order, std::vector<size_t> &leaves)
{
    groupPreOrder(root, order);
    leaves.assign(order.size(), 0);
    for (size_t k = 0; k < order.size(); ++k) order[k]->schedIdx = (int)k;
    const int grp = root->grpID;
    for (size_t k = order.size(); k-- > 0;) {
        Node *n = order[k];
        if (n->children.empty()) { leaves[k] = 1; continue; }
        for (Node *c : n->children)
            if (c->grpID == grp) leaves[k] += leaves[(size_t)c->schedIdx];
    }
}

size_t numLeaves(Node *root)
{
    std::vector<Node *> order;
    std::vector<size_t> leaves;
    leavesBelow(root, order, leaves);
    return leaves[0];
}

// getCentroidEdge / updateCentroidEdge (partitionInfo.cpp:16-38)
Node *centroidEdge(Node *root)
{
    std::vector<Node *> order;
    std::vector<size_t> leaves;
    leavesBelow(root, order, leaves);
    const int grp = root->grpID;
    size_t imbalance = leaves[0];
    const size_t half = std::max<size_t>(1, leaves[0] / 2);
    Node *best = root;
    // post-order: a node is judged when all its children of the group have been
    std::vector<std::pair<Node *, size_t>> work{{root, 0}};
    while (!work.empty()) {
        Node *cur = work.back().first;
        size_t &next = work.back().second;
        if (cur->children.empty()) { work.pop_back(); continue; }      // (a leaf is no candidate: :17)
        while (next < cur->children.size() && cur->children[next]->grpID != grp) ++next;
        if (next < cur->children.size()) { Node *c = cur->children[next++]; work.push_back({c, 0}); continue; }
        const size_t below = leaves[(size_t)cur->schedIdx];
        const size_t off = half > below ? half - below : below - half;
        if (off < imbalance) { best = cur; imbalance = off; }
        work.pop_back();
    }
    return best;
}

// setChildrenGrpID (partitionInfo.cpp:44-52)
void setGroupBelow(Node *root, int from, int to)
{
    std::vector<Node *> work{root};
    while (!work.empty()) {
        Node *cur = work.back();
        work.pop_back();
        if (cur->grpID != from) continue;
        cur->grpID = to;
        for (Node *c : cur->children) work.push_back(c);
    }
}

}  // namespace

// partitionInfo.cpp:54-74
void PartitionInfo::bipartition(Node *root, Node *edge, Node *&tree1Root, Node *&tree2Root)
{
    const int tree1ID = (root->grpID == -1) ? 0 : root->grpID;
    const int tree2ID = (root->grpID == -1) ? 1 : (int)numPartitions + 1;
    numPartitions += 1;
    Node *head = edge->parent;
    const int headID = head->grpID;
    while (head->parent != nullptr && head->parent->grpID == headID) head = head->parent;
    tree1Root = head;
    tree2Root = edge;
    const int tree1Org = tree1Root->grpID;
    setGroupBelow(tree2Root, tree2Root->grpID, tree2ID);
    if (tree1Root->grpID == -1) setGroupBelow(tree1Root, tree1Org, tree1ID);
}

// partitionInfo.cpp:76-110
void PartitionInfo::partitionTree(Node *root)
{
    std::vector<Node *> todo{root};       // (the reference recurses: the split-off part first, then the rest)
    while (!todo.empty()) {
        Node *cur = todo.back();
        todo.pop_back();
        const size_t total = numLeaves(cur);
        if (total <= maxPartitionSize) {
            if (partitionsRoot.empty()) {
                setGroupBelow(cur, cur->grpID, 0);
                partitionsRoot[cur->identifier] = {cur, numLeaves(cur)};
            }
            continue;
        }
        Node *breakEdge = centroidEdge(cur);
        if (breakEdge->identifier == cur->identifier) continue;
        Node *tree1 = nullptr, *tree2 = nullptr;
        bipartition(cur, breakEdge, tree1, tree2);
        const size_t n1 = numLeaves(tree1), n2 = numLeaves(tree2);
        partitionsRoot[tree2->identifier] = {tree2, n2};
        partitionsRoot[tree1->identifier] = {tree1, n1};
        if (n1 > maxPartitionSize) todo.push_back(tree1);
        if (n2 > maxPartitionSize) todo.push_back(tree2);
    }
}

// phylogeny.cpp:13-39: the roots of the subtrees, each under the nearest subtree root above it, in pre-order
Tree *constructTreeFromPartitions(Node *root, PartitionInfo *P)
{
    Tree *T = new Tree();
    std::vector<std::pair<Node *, Node *>> work{{root, nullptr}};      // (a node of the tree, the copy of the nearest subtree root above it)
    while (!work.empty()) {
        Node *node = work.back().first;
        Node *parent = work.back().second;
        work.pop_back();
        if (P->partitionsRoot.count(node->identifier)) {
            Node *copy = T->allNodes.empty() ? new Node(node->identifier, node->branchLength) : new Node(node->identifier, parent, node->branchLength);
            copy->grpID = -1;
            if (T->allNodes.empty()) T->root = copy;
            T->allNodes[copy->identifier] = copy;
            parent = copy;
        }
        for (int i = (int)node->children.size() - 1; i >= 0; --i) work.push_back({node->children[i], parent});
    }
    return T;
}

// tree.cpp:519-526
void updateSubrootInfo(Node *subroot, Tree *subT, int subtreeIdx)
{
    subroot->seqsIncluded.push_back(subtreeIdx);
    subroot->alnLen = subT->root->alnLen;
    subroot->alnNum = (int)subT->root->seqsIncluded.size();
    subroot->msaFreq = subT->root->msaFreq;
    subroot->alnWeight = subT->root->alnWeight;
}

}  // namespace phylogeny
