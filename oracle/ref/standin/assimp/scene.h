// Stand-in for <assimp/scene.h> -- TEST INFRASTRUCTURE ONLY (oracle/_ref).
// The reference's include/model.hpp names these types in the declarations of
// Model's private loader members; nothing the harness links ever defines or
// calls them (Model::Model is supplied empty by oracle/ref/ref_hot.cpp).
#pragma once
struct aiNode;
struct aiScene;
struct aiMesh;
struct aiMaterial;
enum aiTextureType : int;
