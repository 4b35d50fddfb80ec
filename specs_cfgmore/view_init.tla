------------------------------ MODULE view_init ------------------------------
(* Two initial states (the ghost g is 0 or 1) with ONE view: the view applies to the initial states too, one of them is stored. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm view_init
variables g \in {0, 1}, x = 0;

process P \in 1..2
begin
  a: x := x + self;
  b: x := x * 2;
end process

end algorithm *)

View == <<x, pc>>
=============================================================================
